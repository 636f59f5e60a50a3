#!/usr/bin/env python3
"""Measure the species clusters by linkage on one MI355X.  Every timed call runs --repeats times after one warm-up; the
MEDIAN wall milliseconds of the whole Python call are reported beside every run's, and the HIP-event stage milliseconds and counts of
pg_screen_linkage_last of the last run.

  screen   the 32 768-genome synthetic set of tools/screen_index_probe.py at identity 0.80: its kept pairs as a list, the distances from
           the screen identities; the distribution of the component sizes, because it decides everything
  random   64 000 random components of 2 ... 30 nodes (a chain plus as many chords): 10^5 of them would be 1.6 million nodes, beyond the 2^20
           a call takes
  single   one component of 4096 nodes

Every workload is measured under small_limit 0, 16, 32 and 64, and compared with — never with the code under test —
  (a) host   the route this replaces: screen.components_of_pairs, then scipy's linkage and fcluster per component in a Python loop
  (b) small_limit = 0: the heatmap's workgroup kernel doing all the work, the honest baseline for the wave kernel
The partitions of (a) and of every device run must be equal; the report says whether they were.

Every workload runs in a process of its own under a time limit of its own; the first that fails ends the probe.  No time is set in
advance: what is measured is recorded, and what is not is listed under "not_measured".  Writes profiles/screen_linkage_probe.json.

Usage: python tools/screen_linkage_probe.py [--genomes 32768] [--length 20000] [--scale 16] [--components 64000] [--repeats 3]
                                            [--out profiles/screen_linkage_probe.json] [--workload screen|random|single]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402

KMER, THRESHOLD, SEED = 16, 0.80, 20261908      # tools/screen_index_probe.py's: the same synthetic families of 25
LIMITS = (0, 16, 32, 64)
STAGES = ("group_ms", "fill_ms", "small_ms", "large_ms", "cut_ms")
COUNTS = ("n", "entries", "ignored", "components", "worked_components", "largest", "clusters", "batches")
SECONDS = {"screen": 900, "random": 600, "single": 300}


def median_of(fn, repeats):
    """(what the last run returned, the median wall ms, every wall ms) of `repeats` runs after one warm-up."""
    fn()
    walls, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
    return out, round(statistics.median(walls), 3), [round(w, 3) for w in walls]


def host_route(a, b, dist, n, method, cutoff, fill):
    """(a): cluster[v] = the smallest member of v's flat cluster — components by the numpy statement, scipy per component."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from pyani_amd import screen
    root = screen.components_of_pairs(a, b, None, n)[0].astype(np.int64)
    order = np.lexsort((np.arange(n), root))
    heads = np.flatnonzero(root[order] == order)
    start = np.append(heads, n)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    comp = np.searchsorted(heads, pos, side="right") - 1
    local = pos - start[comp]
    live = a != b
    ec = comp[a[live]]
    by = np.argsort(ec, kind="stable")
    ec, ei, ej, ed = ec[by], local[a[live]][by], local[b[live]][by], dist[live][by]
    cuts = np.searchsorted(ec, np.arange(len(heads) + 1))
    cluster = np.arange(n, dtype=np.int64)
    for c in np.flatnonzero(np.diff(start) >= 2).tolist():
        s = int(start[c + 1] - start[c])
        sl = slice(cuts[c], cuts[c + 1])
        D = np.full((s, s), -1.0)
        np.maximum.at(D, (ei[sl], ej[sl]), ed[sl])
        D = np.maximum(D, D.T)
        D[D < 0] = fill
        np.fill_diagonal(D, 0.0)
        lab = fcluster(linkage(squareform(D, checks=False), method), cutoff, "distance")
        nodes = order[start[c]:start[c + 1]]
        first = np.full(lab.max() + 1, s, dtype=np.int64)
        np.minimum.at(first, lab, np.arange(s))
        cluster[nodes] = nodes[first[lab]]
    return cluster.astype(np.int32)


def measure(eng, name, a, b, dist, n, score, method, cutoff, fill, repeats, extra=None):
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    rec = {"workload": name, "nodes": int(n), "entries": int(len(a)), "method": method, "cutoff": cutoff, "fill": fill, **(extra or {})}
    want, h_wall, h_walls = median_of(lambda: host_route(a.astype(np.int64), b.astype(np.int64), dist, n, method, cutoff, fill), repeats)
    rec["host_components_then_scipy"] = {"wall_ms_median": h_wall, "wall_ms_all": h_walls}
    size = np.bincount(np.bincount(np.unique(want, return_inverse=True)[1]))      # (of the clusters; the components' follow from `last`)
    rec["cluster_sizes"] = {str(s): int(c) for s, c in enumerate(size.tolist()) if c}
    rec["device"] = {}
    for limit in LIMITS:
        eng.screen_linkage_set(limit, 0)

        def device():
            nodes = eng.screen_linkage(a, b, dist, n=n, score=score, method=method, cutoff=cutoff, fill=fill)
            return nodes, eng.screen_linkage_last()
        (nodes, last), wall, walls = median_of(device, repeats)
        rec["device"][f"small_limit_{limit}"] = {"wall_ms_median": wall, "wall_ms_all": walls, "equal_to_the_host_route": bool((nodes[1] == want).all()),
                                                 "last": {**{k: last[k] for k in COUNTS}, **{k: round(last[k], 3) for k in STAGES}},
                                                 "linkage_ms": round(last["small_ms"] + last["large_ms"], 3), "host_over_device": round(h_wall / wall, 3)}
        if limit == 0:
            root = nodes[0]
    eng.screen_linkage_set(None, 0)
    eng.screen_linkage_release()
    csize = np.bincount(np.bincount(np.unique(root, return_inverse=True)[1]))
    rec["component_sizes"] = {str(s): int(c) for s, c in enumerate(csize.tolist()) if c}
    base = rec["device"]["small_limit_0"]["linkage_ms"]
    rec["wave_kernel_over_workgroup_kernel"] = {k: round(base / v["linkage_ms"], 3) for k, v in rec["device"].items() if v["linkage_ms"] > 0}
    print(json.dumps(rec), flush=True)
    return rec


def random_components(count, seed):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 31, count)
    start = np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    of = np.repeat(np.arange(count), sizes)
    u = np.flatnonzero(np.arange(n) + 1 < start[of + 1])      # the chains
    x = start[of] + (rng.random(n) * sizes[of]).astype(np.int64)      # one chord per node
    y = start[of] + (rng.random(n) * sizes[of]).astype(np.int64)
    a, b = np.concatenate([u, x]), np.concatenate([u + 1, y])
    label = rng.permutation(n)
    return label[a], label[b], rng.random(len(a)) * 0.3, n


def workload(args):
    from pyani_amd import _lib, screen, synth
    from pyani_amd.engine import Engine
    rec = {"library": _lib.load().pg_version().decode()}
    with Engine(0) as eng:
        if args.workload == "screen":
            n = args.genomes
            t0 = time.perf_counter()
            synth.genome(SEED, n, 0, args.length)
            with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
                data = list(ex.map(lambda g: synth.genome(SEED, n, g, args.length), range(n)))
            ids = [eng.add_genome(s, o) for s, o in data]
            del data
            eng.upload()
            opt = screen.ScreenOptions(THRESHOLD, KMER, args.scale)
            sp = eng.screen_candidates(ids, opt, path="index")
            eng.clear_genomes()
            dist = np.maximum(0.0, 1.0 - sp.identity())
            rec.update(measure(eng, "screen", sp.a, sp.b, dist, n, screen.score_keys(None, sp.sizes), "average", 1.0 - THRESHOLD, 1.0, args.repeats,
                               {"genomes": n, "options": dict(opt._asdict()), "prepare_s": round(time.perf_counter() - t0, 2)}))
        elif args.workload == "random":
            a, b, dist, n = random_components(args.components, 1)
            score = np.random.default_rng(2).integers(0, 1 << 40, n).astype(np.uint64)
            rec.update(measure(eng, "random", a, b, dist, n, score, "average", 0.15, 1.0, args.repeats, {"components_asked": args.components}))
        else:
            rng = np.random.default_rng(3)
            n = 4096
            a = np.concatenate([np.arange(n - 1), rng.integers(0, n, 20 * n)])
            b = np.concatenate([np.arange(1, n), rng.integers(0, n, 20 * n)])
            rec.update(measure(eng, "single", a, b, rng.random(len(a)) * 0.3, n, np.arange(n, dtype=np.uint64), "average", 0.15, 1.0, args.repeats))
    Path(args.out).write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=32768)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--components", type=int, default=64_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_linkage_probe.json"))
    ap.add_argument("--workload", choices=tuple(SECONDS), default=None)
    args = ap.parse_args()
    if args.workload:
        return workload(args)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    report = {"repeats": args.repeats, "timing": "median wall ms of the repeats after one warm-up; stage ms from HIP events of the last run",
              "not_measured": ["method=\"complete\" (the same kernels; the update is a maximum)", "several devices", "run_dereplicate with exact=\"anim\"",
                               "work_bytes other than the default (one batch in every workload)", f"collections beyond {args.genomes} genomes"],
              "workloads": {}}
    for name, seconds in SECONDS.items():
        part = out.with_suffix(f".{name}.part")
        cmd = ["timeout", "-k", "10", str(seconds), sys.executable, str(Path(__file__).resolve()), "--workload", name, "--out", str(part), "--genomes", str(args.genomes),
               "--length", str(args.length), "--scale", str(args.scale), "--components", str(args.components), "--repeats", str(args.repeats)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            report["workloads"][name] = {"failed": rc}
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
            print(f"{name}: exit status {rc}; the probe ends here", flush=True)
            return rc
        report["workloads"][name] = json.loads(part.read_text())
        part.unlink()
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
