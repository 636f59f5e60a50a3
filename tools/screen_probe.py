#!/usr/bin/env python3
"""Measure the screen (pg_screen_matrix) on the benchmark's generator sets and price its estimate against the exact engine.

Per set (C4: 1000 genomes of ~5 Mb, bench.py's ANIm workload, or its first --c4-genomes genomes; C5: 500 genomes of 1 - 12 Mb, the ANIb
workload), at k = 16 and scale 256 and 64:

  screen_matrix        wall seconds of Engine.screen_matrix (second of two runs) and pg_screen_last: keys, distinct entries, groups,
                       pair increments, slices, and the scan / sort + group / count milliseconds; the count kernel's pair increments
                       per second and its share of the three stages
  sketch_pairs         seconds of Engine.sketch_pairs over ALL ordered pairs of the same genomes (sketches built first, timed apart):
                       what the screen replaces for triage
  against the exact    a sample of ordered pairs that includes every family (its first member against all others, both directions) and unrelated pairs,
  engine               through anim_pairs: the largest |screen identity - ANIm identity| where ANIm identity >= 0.90, the lowest
                       screen identity (the larger of the two directions: what candidate_pairs compares) of any sampled pair with ANIm
                       coverage >= 0.5, and — over ALL ordered pairs of the set, by the screen matrix — the share below screen identity
                       0.80 and 0.85 with the share of the exact run's time those pairs would take, EXTRAPOLATED from the seconds per pair
                       the sampled pairs of each class took in the exact engine (anim_pairs on C4, anib_pairs on C5: the benchmark's modes)

No bar is set on any of these.  Writes profiles/screen_probe.json (after every set, so a run that is cut short leaves what it measured).

Usage: python tools/screen_probe.py [--sets C5,C4] [--c4-genomes 1000] [--unrelated 5000] [--out profiles/screen_probe.json]"""
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

KMER = 16
SCALES = (256, 64)


def c5_length(g):
    """SURVEY.md §8(d) set C5, as bench.py states it."""
    return 1_000_000 + (g * 22_045) % 11_000_001


def set_config(name, c4_genomes):
    if name == "C4":
        cfg = synth.SETS["C4"]
        return {"n_generator": cfg["n"], "n": min(c4_genomes, cfg["n"]), "seed": cfg["seed"], "length": lambda g: cfg["L"], "exact": "anim"}
    if name == "C5":
        return {"n_generator": 500, "n": 500, "seed": 20250302, "length": c5_length, "exact": "anib"}
    raise SystemExit(f"unknown set {name}")


def sample_pairs(n, n_generator, n_unrelated, rng):
    """Ordered pairs of genome indices: per family (g % K, K = families of the generator) its first member against every other member and one more pair, both
    directions; then unrelated pairs (two families) drawn at random."""
    K = (n_generator + 24) // 25
    related = []
    for f in range(K):
        members = [g for g in range(f, n, K)]
        if len(members) < 2:
            continue
        picks = {(members[0], m) for m in members[1:]} | {(members[len(members) // 4], members[(3 * len(members)) // 4])}
        for a, b in sorted(picks):
            if a != b:
                related += [(a, b), (b, a)]
    unrelated = set()
    while len(unrelated) < n_unrelated and K > 1:
        a, b = (int(x) for x in rng.integers(0, n, size=2))
        if a % K != b % K:
            unrelated.add((a, b))
    return related, sorted(unrelated)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def probe_set(eng, name, args):
    cfg = set_config(name, args.c4_genomes)
    n = cfg["n"]
    rec = {"set": name, "genomes": n, "generator_genomes": cfg["n_generator"], "seed": cfg["seed"], "kmer": KMER}
    t0 = time.perf_counter()
    with ThreadPoolExecutor(min(16, os.cpu_count() or 2)) as ex:
        data = list(ex.map(lambda g: synth.genome(cfg["seed"], cfg["n_generator"], g, cfg["length"](g)), range(n)))
    ids = np.asarray([eng.add_genome(s, o) for s, o in data], dtype=np.int32)
    lengths = np.array([len(s) for s, _ in data], dtype=np.int64)
    del data
    eng.upload()
    rec["bases"] = int(lengths.sum())
    rec["prepare_seconds"] = round(time.perf_counter() - t0, 2)
    print(name, "resident:", n, "genomes,", rec["bases"], "bases,", rec["prepare_seconds"], "s", flush=True)

    results = {}
    for scale in SCALES:
        eng.screen_matrix(ids, kmer=KMER, scale=scale)                      # first run: allocations, code objects
        (sizes, shared), wall = timed(lambda: eng.screen_matrix(ids, kmer=KMER, scale=scale))
        last = eng.screen_last()
        stages = last["scan_ms"] + last["sort_group_ms"] + last["count_ms"]
        r = dict(last)
        r["wall_seconds"] = round(wall, 4)
        r["pair_increments_per_second"] = round(last["pair_increments"] / (last["count_ms"] * 1e-3), 0) if last["count_ms"] > 0 else None
        r["count_share_of_stages"] = round(last["count_ms"] / stages, 4) if stages > 0 else None
        r["count_share_of_wall"] = round(last["count_ms"] * 1e-3 / wall, 4)
        r["ordered_pairs_per_second"] = round(n * (n - 1) / wall, 0)
        r["mean_size"] = float(sizes.mean())
        rec[f"screen_scale{scale}"] = r
        results[scale] = screen.ScreenResult([str(g) for g in range(n)], KMER, scale, sizes, shared)
        print(name, "scale", scale, json.dumps(r), flush=True)

    # what it replaces for triage: the per-pair sketch over all ordered pairs
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    _, build = timed(lambda: eng.sketch_pairs(ids, np.roll(ids, 1)))      # every genome sketched once (and n pairs)
    _, pairs_s = timed(lambda: eng.sketch_pairs(ids[a], ids[b]))
    rec["sketch_pairs_all_ordered_pairs"] = {"pairs": int(len(a)), "sketch_build_seconds": round(build, 3), "pairs_seconds": round(pairs_s, 3),
                                             "frag_len": 3000, "scale": 16, "kmer": 16}
    print(name, "sketch_pairs", json.dumps(rec["sketch_pairs_all_ordered_pairs"]), flush=True)

    # against the exact engine
    rng = np.random.default_rng(20261905)
    related, unrelated = sample_pairs(n, cfg["n_generator"], args.unrelated, rng)
    sample = related + unrelated
    ra = np.array([p[0] for p in sample]); qa = np.array([p[1] for p in sample])
    exact, anim_s = timed(lambda: eng.anim_pairs(ids[ra], ids[qa]))
    ok = exact["status"] == 0
    anim_identity = np.where(ok, exact["identity"], 0.0)
    anim_cov = np.where(ok, exact["ref_aln_len"] / lengths[ra], 0.0)
    rec["sample"] = {"related_pairs": len(related), "unrelated_pairs": len(unrelated), "anim_seconds": round(anim_s, 3),
                     "anim_pairs_with_alignment": int(ok.sum())}
    for scale in SCALES:
        ident = results[scale].identity().to_numpy()
        directional = ident[ra, qa]
        both = np.maximum(ident, ident.T)
        high = anim_identity >= 0.90
        covered = anim_cov >= 0.5
        cmp_ = {"pairs_with_anim_identity_ge_0.90": int(high.sum()),
                "largest_abs_error_where_anim_identity_ge_0.90": float(np.abs(directional[high] - anim_identity[high]).max()) if high.any() else None,
                "largest_abs_error_of_the_larger_direction_where_anim_identity_ge_0.90": float(np.abs(both[ra, qa][high] - anim_identity[high]).max()) if high.any() else None,
                "lowest_anim_identity_sampled_related": float(anim_identity[:len(related)].min()) if related else None,
                "pairs_with_anim_coverage_ge_0.5": int(covered.sum()),
                "lowest_screen_identity_where_anim_coverage_ge_0.5": float(both[ra, qa][covered].min()) if covered.any() else None,
                "lowest_anim_identity_where_anim_coverage_ge_0.5": float(anim_identity[covered].min()) if covered.any() else None,
                "highest_screen_identity_of_an_unrelated_sampled_pair": float(both[ra, qa][len(related):].max()) if unrelated else None}
        off = ~np.eye(n, dtype=bool)
        for thr in (0.80, 0.85):
            below_all = (both < thr) & off
            below_sample = both[ra, qa] < thr
            # seconds per pair of each class in the exact engine of the set's benchmark mode, on the sample
            times = {}
            for label, mask in (("below", below_sample), ("at_or_above", ~below_sample)):
                if not mask.any():
                    times[label] = None
                    continue
                if cfg["exact"] == "anim":
                    _, s = timed(lambda: eng.anim_pairs(ids[ra[mask]], ids[qa[mask]]))
                else:
                    _, s = timed(lambda: eng.anib_pairs(ids[ra[mask]], ids[qa[mask]]))
                times[label] = s / int(mask.sum())
            n_below, n_above = int(below_all.sum()), int(off.sum()) - int(below_all.sum())
            share_time = None
            if times["below"] is not None and (times["at_or_above"] is not None or n_above == 0):
                tb, ta = n_below * times["below"], n_above * (times["at_or_above"] or 0.0)
                share_time = tb / (tb + ta) if tb + ta > 0 else None
            cmp_[f"below_{thr:.2f}"] = {"share_of_ordered_pairs": n_below / int(off.sum()), "ordered_pairs": n_below,
                                        "exact_mode": cfg["exact"], "sample_seconds_per_pair_below": times["below"],
                                        "sample_seconds_per_pair_at_or_above": times["at_or_above"],
                                        "share_of_exact_time_extrapolated_from_the_sample": share_time,
                                        "sampled_pairs_below_with_anim_coverage_ge_0.5": int((below_sample & covered).sum())}
        rec[f"against_exact_scale{scale}"] = cmp_
        print(name, "scale", scale, "against the exact engine", json.dumps(cmp_), flush=True)
    eng.clear_genomes()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="C5,C4")
    ap.add_argument("--c4-genomes", type=int, default=1000)
    ap.add_argument("--unrelated", type=int, default=5000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "screen_probe.json"))
    args = ap.parse_args()
    report = {"library": _lib.load().pg_version().decode(), "sets": {}}
    out = Path(args.out)
    if out.exists():      # a later run of one set keeps the other's figures
        try:
            report["sets"] = json.loads(out.read_text()).get("sets", {})
        except ValueError:
            pass
    with Engine(0) as eng:
        for name in args.sets.split(","):
            report["sets"][name] = probe_set(eng, name, args)
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
