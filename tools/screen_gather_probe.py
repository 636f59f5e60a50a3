#!/usr/bin/env python3
"""Measure the screen's gather on one MI355X.

  collection  the synthetic set of tools/screen_search_probe.py: 32 768 + 1024 genomes (pyani_amd.synth, families of 25, --length bases,
              scale --scale), every 33rd held out; the collection is the other 32 768, indexed once.
  queries     mixtures: --members (4, 32, 256) held-out genomes joined into ONE multi-record genome, and --queries (1, 64) such mixtures
              per call (a mixture takes its members at an even stride through the 1024 held-out genomes, each mixture from another start).
  measured    per (members, queries), best of --repeats after one warm-up: the wall milliseconds of Engine.screen_gather (the count with
              its entries kept, the rounds, the rows read back) and of Engine.screen_search over the same queries, for scale; of the last
              run the counters and HIP-event milliseconds of pg_screen_gather_last and the count's stages of pg_screen_search_last.
  compaction  the same gather with the entries never compacted (PYANI_GATHER_COMPACT=0, a development switch), for the decision
              recorded in DESIGN.md.
  host        THE SAME GREEDY LOOP restated on the host (scipy.sparse over the k-mer incidence), timed WITHOUT building the incidence —
              the product has no host sampler, so the sets come from the tests' numpy statement, and only for the db genomes that share a
              k-mer with the query (the others can never win).  Run for one mixture (queries = 1) of the --host-members sizes.  It is a
              restatement for scale, not the parent commit: the parent has no gather.

No time is set in advance: what is measured is recorded.  Writes profiles/screen_gather_probe.json.

Usage: python tools/screen_gather_probe.py [--members 4,32,256] [--queries 1,64] [--host-members 4,32,256] [--length 20000] [--scale 16]
                                           [--min-unique 20] [--repeats 3] [--out profiles/screen_gather_probe.json]"""
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

KMER, SEED, N_DB, N_HELD = 16, 20261908, 32768, 1024
SEARCH_IDENTITY = 0.80


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


def rounded(last):
    return {k: (round(v, 3) if k.endswith("_ms") else v) for k, v in last.items()}


def host_greedy(inc, need, max_ranks):
    """The rounds over a scipy CSR incidence (db genomes x the query's matched k-mers): rows [(b, unique)]."""
    alive = np.ones(inc.shape[1], dtype=np.int64)
    rows = []
    while len(rows) < max_ranks:
        left = inc @ alive
        w = int(np.argmax(left))      # (the first of the largest: the smallest b)
        if left[w] < need:
            break
        rows.append((w, int(left[w])))
        alive[inc.indices[inc.indptr[w]:inc.indptr[w + 1]]] = 0
    return rows


def host_route(eng, data, db, members, q_id, opt, repeats):
    """One mixture on the host: the incidence from the numpy statement of the tests, then the greedy loop, timed on its own."""
    import scipy.sparse as sp
    from tests import screen_cases as scr
    t0 = time.perf_counter()
    size = eng.screen_gather_count([q_id])
    hits = eng.screen_search_fetch()[0]
    cols = np.flatnonzero(hits)      # positions in the index call; the others share nothing with the query
    query = np.unique(np.concatenate([scr.genome_set(*data[g], opt.kmer, opt.scale) for g in members]))
    ri, ci = [], []
    for r, c in enumerate(cols.tolist()):
        j = np.searchsorted(query, np.intersect1d(query, scr.genome_set(*data[db[c]], opt.kmer, opt.scale), assume_unique=True))
        ri.append(np.full(len(j), r, dtype=np.int64))
        ci.append(j)
    inc = sp.csr_matrix((np.ones(sum(len(x) for x in ci), dtype=np.int64), (np.concatenate(ri), np.concatenate(ci))), shape=(len(cols), len(query)))
    build_s = time.perf_counter() - t0
    need = int(screen.gather_thresholds(size, opt.min_unique, opt.min_fraction)[0])
    rows, rec = timed(lambda: host_greedy(inc, need, opt.max_ranks), repeats)
    rec["incidence_seconds_not_counted"] = round(build_s, 2)
    rec["db_genomes_with_a_hit"], rec["incidence_entries"] = int(len(cols)), int(inc.nnz)
    return [(int(cols[w]), u) for w, u in rows], rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,32,256")
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--host-members", default="4,32,256")
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--min-unique", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_gather_probe.json"))
    args = ap.parse_args()
    os.environ["PYANI_DEV_KNOBS"] = "1"      # for the compaction switch alone
    os.environ.pop("PYANI_GATHER_COMPACT", None)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    opt = screen.GatherOptions(KMER, args.scale, args.min_unique)
    n = N_DB + N_HELD
    host_members = {int(x) for x in args.host_members.split(",") if x}
    report = {"library": _lib.load().pg_version().decode(), "options": dict(opt._asdict()), "synthetic_length": args.length, "db_genomes": N_DB, "cases": []}
    with Engine(0) as eng:
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            data = list(ex.map(lambda g: synth.genome(SEED, n, g, args.length), range(n)))
        held = [g for g in range(n) if g % 33 == 32]
        held_set = set(held)
        db = [g for g in range(n) if g not in held_set]
        db_ids = [eng.add_genome(*data[g]) for g in db]
        eng.upload()
        _, report["index"] = timed(lambda: eng.screen_search_index(db_ids, KMER, args.scale), 1)
        report["index"]["index_bytes_held"] = eng.screen_search_last()["index_bytes"]
        eng.clear_genomes()      # the index stays; the queries take the store
        report["prepare_seconds"] = round(time.perf_counter() - t0, 2)
        print("index resident:", report["index"], flush=True)
        for m in (int(x) for x in args.members.split(",") if x):
            for q in (int(x) for x in args.queries.split(",") if x):
                eng.clear_genomes()
                mixes = [[held[(j * 17 + i * (N_HELD // m)) % N_HELD] for i in range(m)] for j in range(q)]
                q_ids = [eng.add_genome(*join([data[g] for g in mix])) for mix in mixes]
                eng.upload()
                rec = {"members": m, "queries": q}
                res, rec["gather"] = timed(lambda: eng.screen_gather(q_ids, opt), args.repeats)
                # the stages of the last chunk's calls: gather_chunks drops them at its end, so one chunk is run again by hand
                sizes = eng.screen_gather_count(q_ids)
                need = screen.gather_thresholds(sizes, opt.min_unique, opt.min_fraction)
                _, rec["rounds_only"] = timed(lambda: eng.screen_gather_rows(need, opt.max_ranks), args.repeats)
                rec["gather"]["last"] = rounded(eng.screen_gather_last())
                count = eng.screen_search_last()
                rec["gather"]["count_stages"] = rounded({k: count[k] for k in ("query_keys", "lookups", "matched", "increments", "scan_ms", "sort_group_ms", "lookup_ms", "count_ms")})
                rec["gather"]["rows"] = int(len(res.query))
                rec["gather"]["rows_per_query"] = round(len(res.query) / q, 2)
                rec["gather"]["explained_over_matched"] = round(float(res.unique.sum()) / max(1, int(res.matched.sum())), 4)
                os.environ["PYANI_GATHER_COMPACT"] = "0"
                rows_nc, rec["rounds_only_without_compaction"] = timed(lambda: eng.screen_gather_rows(need, opt.max_ranks), args.repeats)
                rec["rounds_only_without_compaction"]["last"] = rounded(eng.screen_gather_last())
                os.environ.pop("PYANI_GATHER_COMPACT")
                rec["compaction_changes_nothing"] = bool(all((x == y).all() for x, y in zip(rows_nc, (res.query, res.db, res.unique, res.total))))
                _, rec["search"] = timed(lambda: eng.screen_search(q_ids, screen.ScreenOptions(SEARCH_IDENTITY, KMER, args.scale)), args.repeats)
                if q == 1 and m in host_members:
                    rows, rec["host_restatement"] = host_route(eng, data, db, mixes[0], q_ids[0], opt, args.repeats)
                    rec["host_restatement"]["equal"] = rows == list(zip(res.db.tolist(), res.unique.tolist()))
                    rec["host_over_rounds_only"] = round(rec["host_restatement"]["wall_ms_best"] / rec["rounds_only"]["wall_ms_best"], 3)
                report["cases"].append(rec)
                print(json.dumps(rec), flush=True)
                out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
        eng.screen_search_index_release()
    print("wrote", out)


if __name__ == "__main__":
    main()
