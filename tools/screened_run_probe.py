#!/usr/bin/env python3
"""Measure the screen's selection on the device and what a screen in front of run_anim / run_anib saves, on one MI355X.

  selection   n = 1000 and n = 8192: a random symmetric matrix (sizes 15 000 ... 25 000, about 1 % of the pairs related) is loaded
              (Engine.screen_load) and selected at identity 0.80, k = 16.  device_ms = Engine.screen_select (both kernel passes, the scan
              and the read-back of the kept triples), best and median of --repeats runs after one warm-up; host_ms = the path it
              replaces, which stays in the tree unchanged: the read-back of the n x n matrix (Engine.screen_fetch) plus
              ScreenResult.candidate_pairs, timed apart.  The two lists are compared and must be equal.
  runs        one synthetic collection of --families families (pyani_amd.synth; --genomes genomes of --length bases): run_anim
              (skip_zero) and run_anib, unscreened and with ScreenOptions(0.80, scale=--scale): wall seconds, kept and total ordered
              pairs, and whether the kept pairs' results equal the unscreened run's.

No ratio is set in advance: what is measured is recorded.  Writes profiles/screened_run_probe.json.

Usage: python tools/screened_run_probe.py [--sizes 1000,8192] [--repeats 5] [--genomes 60] [--families 6] [--length 1000000] [--scale 64]
                                          [--out profiles/screened_run_probe.json]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np      # noqa: E402

from pyani_amd import _lib, screen, synth      # noqa: E402
from pyani_amd.engine import Engine            # noqa: E402

KMER, THRESHOLD = 16, 0.80


def random_matrix(n, rng):
    """sizes and a symmetric shared matrix: unrelated pairs share a few chance k-mers, about 1 % of the pairs 30 - 100 % of the smaller size."""
    sizes = rng.integers(15_000, 25_001, n).astype(np.int64)
    cap = np.minimum.outer(sizes, sizes)
    m = rng.integers(0, 40, (n, n)).astype(np.int64)
    related = rng.random((n, n)) < 0.01
    m = np.where(related, (cap * (0.3 + 0.7 * rng.random((n, n)))).astype(np.int64), m)
    m = np.triu(m, 1)
    m = m + m.T
    m[np.arange(n), np.arange(n)] = sizes
    return sizes.astype(np.uint32), m.astype(np.uint32)


def ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def probe_selection(eng, n, repeats):
    rng = np.random.default_rng(20261906 + n)
    sizes, shared = random_matrix(n, rng)
    _, load_ms = ms(lambda: eng.screen_load(shared))
    (need, thresholds_ms) = ms(lambda: screen.identity_thresholds(sizes, KMER, THRESHOLD, 2))
    eng.screen_select(need)      # warm-up: code objects, the output buffers
    device = []
    for _ in range(repeats):
        got, t = ms(lambda: eng.screen_select(need))
        device.append(t)
    fetch, host_pairs = [], []
    for _ in range(max(1, min(repeats, 3))):
        back, t = ms(eng.screen_fetch)
        fetch.append(t)
        res = screen.ScreenResult([str(i) for i in range(n)], KMER, 256, sizes, back)
        want, t = ms(lambda: res.candidate_pairs(THRESHOLD))
        host_pairs.append(t)
    eng.screen_release()
    equal = list(zip(got[0].tolist(), got[1].tolist())) == want
    rec = {"n": n, "ordered_pairs": n * (n - 1), "kept": int(len(got[0])), "kept_share": len(got[0]) / (n * (n - 1)), "equal_to_candidate_pairs": bool(equal),
           "load_ms": round(load_ms, 3), "identity_thresholds_ms": round(thresholds_ms, 3),
           "device_select_and_read_ms": {"best": round(min(device), 3), "median": round(statistics.median(device), 3)},
           "host_fetch_ms": {"best": round(min(fetch), 3), "median": round(statistics.median(fetch), 3)},
           "host_candidate_pairs_ms": {"best": round(min(host_pairs), 3), "median": round(statistics.median(host_pairs), 3)}}
    rec["host_path_ms_best"] = round(min(fetch) + min(host_pairs), 3)
    rec["matrix_bytes"] = int(shared.nbytes)
    rec["streamed_GB_per_s_at_best"] = round(2 * shared.nbytes / (min(device) * 1e-3) / 1e9, 1)      # (two passes; includes the scan and the read-back)
    return rec


def probe_runs(eng, args):
    from pyani_amd.subcmd_anib import run_anib
    from pyani_amd.subcmd_anim import run_anim
    n_gen = 25 * args.families      # pyani_amd.synth: families of the generator = (n + 24) // 25, genome g in family g % families
    opt = screen.ScreenOptions(THRESHOLD, scale=args.scale)
    rec = {"genomes": args.genomes, "families": args.families, "length": args.length, "options": dict(opt._asdict()),
           "total_ordered_pairs": args.genomes * (args.genomes - 1)}
    with tempfile.TemporaryDirectory() as tmp:
        indir = Path(tmp)
        for g in range(args.genomes):
            seq, off = synth.genome(20261907, n_gen, g, args.length)
            synth.write_fasta(indir / f"{synth.genome_name(g)}.fna", seq, off, synth.genome_name(g))
        for mode, run, kw in (("anim", run_anim, {"skip_zero": True}), ("anib", run_anib, {})):
            eng.clear_genomes()
            run(indir, engine=eng, **kw)      # warm-up: code objects, scratch
            plain, plain_ms = ms(lambda: run(indir, engine=eng, **kw))
            run(indir, engine=eng, screen=opt, **kw)
            scr, scr_ms = ms(lambda: run(indir, engine=eng, screen=opt, **kw))
            kept = len(scr.screened.a)
            same = all(k in plain.results and plain.results[k] == v for k, v in scr.results.items())
            lost = [k for k in plain.results if k not in scr.results]
            rec[mode] = {"unscreened_wall_s": round(plain_ms / 1e3, 4), "screened_wall_s": round(scr_ms / 1e3, 4), "kept_pairs": kept,
                         "pairs_with_a_result_unscreened": len(plain.results), "pairs_with_a_result_screened": len(scr.results),
                         "kept_results_equal_the_unscreened": bool(same),
                         "highest_identity_of_a_dropped_pair_with_a_result": (max(float(plain.results[k][2]) * (0.01 if mode == "anib" else 1.0) for k in lost) if lost else None)}
            print(mode, json.dumps(rec[mode]), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,8192")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--genomes", type=int, default=60)
    ap.add_argument("--families", type=int, default=6)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--scale", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screened_run_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "kmer": KMER, "min_identity": THRESHOLD, "selection": [], "runs": None}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with Engine(0) as eng:
        for n in (int(x) for x in args.sizes.split(",") if x):
            report["selection"].append(probe_selection(eng, n, args.repeats))
            print("selection", json.dumps(report["selection"][-1]), flush=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
        report["runs"] = probe_runs(eng, args)
        out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
