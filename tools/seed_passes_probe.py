"""What seeding in passes (pyani_amd/csrc/pg_seed_plan.h) costs at a user's sizes, on seeded synthetic inputs.

  (a) anib_subject   ANIb with a 1 Mb query against a 20 Mb subject (coarse groups of ~9 800 entries: two passes) and against a 12 Mb
                     subject (~5 900: one pass), both random sequence carrying three diverged copies of the query: seconds per
                     subject Mb of the call and of the seeding kernel.
  (b) anim_repeat    the tandem genome of tests/test_seed_passes_gpu.py (300 kb + 9000 copies of a 40-base unit: fine groups of 9000
                     and 18 000 equal keys, two and three passes) as the reference of two relatives through anim_pairs, beside its
                     repeat-free twin (the tandem replaced by random sequence): the seeding kernel's time of each.
  (c) anim_150mb     one ANIm pair with a 150 Mb reference (fine groups of ~9 200 entries: two passes) against a 5 Mb relative of a
                     5 Mb stretch embedded in it.

Every call's pair status is recorded: a PG_E_CAPACITY (-9) of a stage AFTER seeding at these sizes is a finding, not a failure of
the probe.  Times: the median wall time of --repeats calls after one warm-up, the engine synchronised before each clock reading; the
seeding kernel's time from the library's own stage timer (pg_profile_*, device events), in a repeat of its own.  Writes
profiles/seed_passes_probe.json (or --out); a "headline" entry already in that file (the benchmark runs, added by hand) is kept.

    python tools/seed_passes_probe.py [--out FILE] [--repeats 3] [--only a,b,c]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _random(rng, n):
    return ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]


def _measure(eng, fn, repeats):
    """fn() once to warm up (seed lists, scratch growth), `repeats` timed calls, one more under the stage timer."""
    from pyani_amd import _lib
    out = fn()
    times = []
    for _ in range(repeats):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        times.append(time.perf_counter() - t0)
    eng.profile_reset()
    eng.profile_config(kernel_mask=1 << _lib.K_ANIM_SEED, every_n=1)
    eng.profile_enable(True)
    fn()
    eng.sync()
    eng.profile_enable(False)
    seed_ms, launches = eng.profile_get(_lib.K_ANIM_SEED)
    return out, {"call_s": statistics.median(times), "call_all_s": times, "seed_kernel_ms": seed_ms, "seed_kernel_launches": int(launches)}


def _guarded(report, key, fn):
    from pyani_amd._lib import PyaniGpuError
    try:
        report[key] = fn()
    except PyaniGpuError as e:   # a refusal at these sizes is what the probe is here to find
        report[key] = {"error_code": e.code, "error": str(e)}
    print(key, json.dumps(report[key])[:400], flush=True)


def probe_anib_subject(eng, repeats):
    from pyani_amd import synth
    qry = synth.genome(77, 4, 0, 1_000_000)
    out = []
    for mb in (12, 20):
        rng = np.random.default_rng(5)
        big = _random(rng, mb * 1_000_000)
        for k, at in enumerate((1_000_000, mb * 500_000, (mb - 2) * 1_000_000)):
            cp, _ = synth.genome(77, 4, 1 + k, 1_000_000)      # descendants of the query's ancestor
            big[at:at + len(cp)] = cp
        eng.clear_genomes()
        q = eng.add_genome(*qry)
        s = eng.add_genome(big, np.array([0, len(big) // 2, len(big)], dtype=np.uint64))
        eng.upload()
        res, t = _measure(eng, lambda: eng.anib_pairs([q], [s]), repeats)
        r = res[0]
        t.update({"subject_mb": mb, "passes_expected": 2 if mb == 20 else 1, "status": int(r["status"]), "n_frags": int(r["n_frags"]),
                  "n_kept": int(r["n_kept"]), "pid": float(r["pid"]), "call_s_per_subject_mb": t["call_s"] / mb,
                  "seed_kernel_ms_per_subject_mb": t["seed_kernel_ms"] / mb})
        out.append(t)
    return out


def probe_anim_repeat(eng, repeats):
    from pyani_amd import synth
    fam = [synth.genome(20250702, 4, g, 300_000) for g in range(3)]
    head = fam[0][0][:300_000]
    off = np.array([int(x) for x in fam[0][1] if int(x) < len(head)] + [len(head) + 360_000], dtype=np.uint64)
    unit = ACGT[np.random.RandomState(5).randint(0, 4, 40)]
    tails = {"tandem_9000x40": np.tile(unit, 9000), "repeat_free_twin": _random(np.random.default_rng(9), 360_000)}
    out = {}
    for name, tail in tails.items():
        eng.clear_genomes()
        ref = eng.add_genome(np.concatenate([head, tail]), off)
        b, c = eng.add_genome(*fam[1]), eng.add_genome(*fam[2])
        eng.upload()
        res, t = _measure(eng, lambda: eng.anim_pairs([ref, ref], [b, c]), repeats)
        t.update({"status": [int(x) for x in res["status"]], "n_alignments": [int(x) for x in res["n_alignments"]],
                  "identity": [float(x) for x in res["identity"]]})
        out[name] = t
    out["seed_kernel_tandem_over_twin"] = out["tandem_9000x40"]["seed_kernel_ms"] / out["repeat_free_twin"]["seed_kernel_ms"]
    return out


def probe_anim_150mb(eng, repeats):
    from pyani_amd import synth
    rel = synth.genome(20250703, 2, 0, 5_000_000)
    inside, _ = synth.genome(20250703, 2, 1, 5_000_000)
    big = _random(np.random.default_rng(15), 150_000_000)
    big[70_000_000:70_000_000 + len(inside)] = inside
    eng.clear_genomes()
    ref = eng.add_genome(big, np.array([0, len(big)], dtype=np.uint64))
    q = eng.add_genome(*rel)
    eng.upload()
    res, t = _measure(eng, lambda: eng.anim_pairs([ref], [q]), repeats)
    r = res[0]
    t.update({"reference_mb": 150, "query_mb": 5, "status": int(r["status"]), "n_alignments": int(r["n_alignments"]),
              "ref_aln_len": int(r["ref_aln_len"]), "identity": float(r["identity"])})
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seed_passes_probe.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    args = ap.parse_args()
    from pyani_amd.engine import Engine
    out = Path(args.out)
    report = json.loads(out.read_text()) if out.exists() else {}
    report.update({"repeats": args.repeats,
                   "statistic": "call_s: median wall seconds after one warm-up, engine synchronised before each clock reading; "
                                "seed_kernel_ms: the library's stage timer (device events) over one further call"})
    parts = {"a": ("anib_subject", probe_anib_subject), "b": ("anim_repeat", probe_anim_repeat), "c": ("anim_150mb", probe_anim_150mb)}
    with Engine(0) as eng:
        for k in args.only.split(","):
            name, fn = parts[k]
            _guarded(report, name, lambda: fn(eng, args.repeats))
            out.parent.mkdir(parents=True, exist_ok=True)
            out.write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")   # (after every part: a later part may be refused)


if __name__ == "__main__":
    main()
