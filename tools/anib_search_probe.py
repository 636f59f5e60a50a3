#!/usr/bin/env python3
"""What the ANIb search mode "all_diagonals" (pg_anib_set_search) changes and what it costs, on an MI355X.

  python tools/anib_search_probe.py [--out profiles/anib_search_probe.json] [--cache DIR] [--parent-steps A.json B.json]
  python tools/anib_search_probe.py --step-only [--tree PATH] --out STEP.json      # the C5-shaped step in default mode, nothing else
  python tools/anib_search_probe.py --references-only --cache DIR                   # no GPU: fill the cache of host-side references

For the 30 ordered pairs of synth.genome(20250302, 6, g, 150_000) and the 12 ordered pairs of the four Caulobacter genomes
(tests/golden/genomes/caulobacter), in both modes: the rows parse_blast_tab uses (pyani/anib.py:641-649) that are identical to the
independent blastn oracle's (oracle/blastn_oracle.cpp), the rows used on one side only, the pair tuple beside BLAST+'s own table
where the reference's tests hold one (tests/golden/anib), and the anib_frag_kernel time of the call (profile slot PG_K_ANIB_FRAG).
Before anything is timed the mode's tables of the 30 synthetic pairs must equal the host statement's (oracle/anib_cpu.cpp with
ANIB_ALL_DIAGS set), row for row.

The C5-shaped step: genomes 0 .. 49 of the C5 generator (seed 20250302, n = 500, L_g = 1 000 000 + (g * 22 045 mod 11 000 001)), the
fragments of genomes 0 .. 9 against the other 49 each — 490 ordered pairs in one anib_pairs call.  Wall time per step, median of
--repeats (5) after one warm-up call that builds the seed lists, profiling off; then one profiled call for the kernel time.

--step-only times that step in default mode with the package under --tree (default: this tree): run on the parent commit's tree
twice and on this one, in one session, it gives the default mode's cost beside the parent's run-to-run spread; --parent-steps
merges the parent's two files into the report.

--cache DIR keeps the host-side references (oracle tables, host-statement tables) as .npy files: they do not depend on the GPU,
so they can be computed ahead (--references-only) and only read here."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CAULOBACTER = ["NC_002696", "NC_010338", "NC_011916", "NC_014100"]
C5_SEED, C5_N, C5_GENOMES, C5_QUERIES = 20250302, 500, 50, 10


class _Env:      # what tests/anib_search_cases.host_pair needs of pytest's monkeypatch
    @staticmethod
    def setenv(k, v):
        os.environ[k] = v

    @staticmethod
    def delenv(k, raising=True):
        os.environ.pop(k, None)


def c5_length(g):
    return 1_000_000 + (g * 22_045) % 11_000_001


def cached(cache, name, make):
    if cache is None:
        return make()
    f = Path(cache) / f"{name}.npy"
    if f.is_file():
        return np.load(f)
    rows = make()
    f.parent.mkdir(parents=True, exist_ok=True)
    np.save(f, rows)
    return rows


def time_c5_step(eng, K_FRAG, repeats):
    """{"step_ms": [...], "median_ms", "frag_kernel_ms"} of the C5-shaped step in the engine's current mode."""
    from pyani_amd import synth
    with ThreadPoolExecutor(8) as ex:
        data = list(ex.map(lambda g: synth.genome(C5_SEED, C5_N, g, c5_length(g)), range(C5_GENOMES)))
    eng.clear_genomes()
    ids = [eng.add_genome(*d) for d in data]
    eng.upload()
    qs = [ids[q] for q in range(C5_QUERIES) for s in range(C5_GENOMES) if s != q]
    ss = [ids[s] for q in range(C5_QUERIES) for s in range(C5_GENOMES) if s != q]
    eng.profile_enable(False)
    first = eng.anib_pairs(qs, ss)      # warm-up: seed lists, word indices, scratch
    eng.sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        rec = eng.anib_pairs(qs, ss)
        eng.sync()
        times.append(1e3 * (time.perf_counter() - t0))
        assert [tuple(r) for r in rec] == [tuple(r) for r in first]
    eng.profile_reset()
    eng.profile_config(kernel_mask=1 << K_FRAG, every_n=1)
    eng.profile_enable(True)
    eng.anib_pairs(qs, ss)
    frag_ms, launches = eng.profile_get(K_FRAG)
    eng.profile_enable(False)
    return {"pairs": len(qs), "related_pairs": int(sum(int(r["n_kept"]) > 0 for r in first)), "fragments": int(sum(int(r["n_frags"]) for r in first)),
            "step_ms": [round(t, 2) for t in times], "median_ms": round(statistics.median(times), 2),
            "frag_kernel_ms": round(frag_ms, 2), "frag_kernel_launches": int(launches)}, first


def step_only(a):
    tree = Path(a.tree).resolve() if a.tree else ROOT
    sys.path.insert(0, str(tree))
    from pyani_amd import _lib
    from pyani_amd.engine import Engine
    assert Path(_lib.LIB_PATH).resolve().parent.parent == tree, (_lib.LIB_PATH, tree)
    with Engine(0) as eng:
        rep, _ = time_c5_step(eng, _lib.K_ANIB_FRAG, a.repeats)
    rep["tree"] = a.label or tree.name
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(rep, indent=1) + "\n")
    print(json.dumps(rep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "anib_search_probe.json"))
    ap.add_argument("--cache", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--references-only", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default=None)
    ap.add_argument("--parent-steps", nargs=2, default=None)
    ap.add_argument("--skip-real", action="store_true", help="leave the 12 Caulobacter pairs out")
    a = ap.parse_args()
    if a.step_only:
        return step_only(a)
    for p in (ROOT, ROOT / "oracle", ROOT / "tools"):
        sys.path.insert(0, str(p))
    import blastn_oracle
    import blastn_oracle_agreement as agreement
    from anib_product_vs_oracle import side_by_side, tuples
    from tests import anib_search_cases as cases
    ON, OFF = "all_diagonals", "seeds"
    syn = cases.genomes()
    syn_pairs = [(q, s) for q in range(cases.N) for s in range(cases.N) if q != s]
    gdir = ROOT / "tests" / "golden" / "genomes" / "caulobacter"
    real = {} if a.skip_real else {n: agreement.read_fasta_gz(gdir / f"{n}.fna.gz") for n in CAULOBACTER}
    real_pairs = [(q, s) for q in real for s in real if q != s]

    def oracle_rows(name, Q, S):
        return cached(a.cache, f"oracle_{name}", lambda: blastn_oracle.blastn_pair(Q, S))

    def host_mode_rows(q, s):
        return cached(a.cache, f"host_{ON}_{q}_{s}", lambda: cases.host_pair(_Env, syn[q], syn[s], ON))

    if a.references_only:
        assert a.cache
        for q, s in syn_pairs:
            oracle_rows(f"syn{q}_syn{s}", syn[q], syn[s])
            host_mode_rows(q, s)
        for q, s in real_pairs:
            t0 = time.time()
            oracle_rows(f"{q}_{s}", real[q], real[s])
            print(f"oracle {q} vs {s}: {time.time() - t0:.0f} s", flush=True)
        return

    from pyani_amd import _lib
    from pyani_amd.engine import Engine
    K = _lib.K_ANIB_FRAG
    report = {"tool": "tools/anib_search_probe.py", "modes": [OFF, ON]}

    def measure(eng, q, s, name, Q, S):
        """Both modes of one pair: agreement with the oracle, one-sided rows, tuple, kernel time."""
        uo = agreement.used_rows(tuples(oracle_rows(name, Q, S)))
        out = {}
        for m in (OFF, ON):
            eng.anib_set_search(m)
            eng.profile_reset()
            rows = eng.anib_pair_rows(q, s)
            ms, _ = eng.profile_get(K)
            rep = side_by_side(agreement.used_rows(tuples(rows)), uo)
            out[m] = {"rows": len(rows), "used_rows": rep["used_rows_product"], "identical_to_oracle": rep["identical"],
                      "only_product": rep["only_product"], "only_oracle": rep["only_other"], "tuple": rep["tuple_product"],
                      "frag_kernel_ms": round(ms, 3)}
            out["_rows_" + m] = rows
        eng.anib_set_search(OFF)
        out["oracle_used_rows"] = len(uo)
        out["oracle_tuple"] = agreement.reduce_used(uo)
        return out

    with Engine(0) as eng:
        ids = [eng.add_genome(*g) for g in syn]
        eng.upload()
        # 1. the mode's tables equal the host statement's before anything is timed
        eng.anib_set_search(ON)
        for q, s in syn_pairs:
            got, want = eng.anib_pair_rows(ids[q], ids[s]), host_mode_rows(q, s)
            if cases.rows_of(got) != cases.rows_of(want):
                raise SystemExit(f"mode {ON}: the GPU's table of synthetic pair ({q}, {s}) differs from the host statement's ({len(got)} vs {len(want)} rows)")
        eng.anib_set_search(OFF)
        report["gpu_equals_host_statement_in_the_mode"] = f"{len(syn_pairs)} of {len(syn_pairs)} synthetic pairs, row for row"
        print("GPU == host statement on the synthetic pairs", flush=True)
        eng.profile_config(kernel_mask=1 << K, every_n=1)
        eng.profile_enable(True)
        # 2. the synthetic pairs
        table, tot = [], {m: {"identical_to_oracle": 0, "frag_kernel_ms": 0.0} for m in (OFF, ON)}
        used = changed_total = 0
        for q, s in syn_pairs:
            r = measure(eng, ids[q], ids[s], f"syn{q}_syn{s}", syn[q], syn[s])
            a_, b_ = cases.rows_of(r.pop("_rows_" + OFF)), cases.rows_of(r.pop("_rows_" + ON))
            r["rows_the_mode_changes"] = len(set(b_) - set(a_))
            r["query"], r["subject"], r["oracle_identity"] = q, s, round(r["oracle_tuple"][2], 2)
            table.append(r)
            used += r["oracle_used_rows"]
            changed_total += r["rows_the_mode_changes"]
            for m in (OFF, ON):
                tot[m]["identical_to_oracle"] += r[m]["identical_to_oracle"]
                tot[m]["frag_kernel_ms"] = round(tot[m]["frag_kernel_ms"] + r[m]["frag_kernel_ms"], 3)
        report["synthetic"] = {"genomes": "synth.genome(20250302, 6, g, 150_000)", "pairs": table,
                               "total": {"oracle_used_rows": used, "rows_the_mode_changes": changed_total, **tot}}
        print(json.dumps(report["synthetic"]["total"]), flush=True)
        # 3. the Caulobacter pairs
        if real:
            eng.clear_genomes()
            rid = {n: eng.add_genome(*real[n]) for n in real}
            eng.upload()
            eng.anib_set_search(OFF)
            eng.profile_enable(False)
            eng.anib_pairs([rid[q] for q, _ in real_pairs], [rid[s] for _, s in real_pairs])      # warm-up: seed lists, word indices
            eng.profile_enable(True)
            table = []
            for q, s in real_pairs:
                r = measure(eng, rid[q], rid[s], f"{q}_{s}", real[q], real[s])
                by_mode = {m: r.pop("_rows_" + m) for m in (OFF, ON)}
                r["rows_the_mode_changes"] = len(set(cases.rows_of(by_mode[ON])) - set(cases.rows_of(by_mode[OFF])))
                r["query"], r["subject"] = q, s
                gold = ROOT / "tests" / "golden" / "anib" / f"{q}_vs_{s}.blast_tab.gz"
                if gold.is_file():
                    ub = agreement.used_rows(agreement.blast_rows(gold, agreement.record_names(gdir / f"{s}.fna.gz")))
                    r["blastplus_tuple"] = agreement.reduce_used(ub)
                    r["blastplus_used_rows"] = len(ub)
                    for m in (OFF, ON):
                        r[m]["identical_to_blastplus"] = side_by_side(agreement.used_rows(tuples(by_mode[m])), ub)["identical"]
                table.append(r)
                print(f"{q} vs {s}: identical to the oracle {r[OFF]['identical_to_oracle']} -> {r[ON]['identical_to_oracle']} of {r['oracle_used_rows']}; "
                      f"kernel {r[OFF]['frag_kernel_ms']} -> {r[ON]['frag_kernel_ms']} ms", flush=True)
            report["caulobacter"] = {"pairs": table}
        eng.profile_enable(False)
        # 4. the C5-shaped step in both modes
        steps = {}
        for m in (OFF, ON):
            eng.anib_set_search(m)
            steps[m], _ = time_c5_step(eng, K, a.repeats)
        eng.anib_set_search(OFF)
        steps["mode_over_default"] = round(steps[ON]["median_ms"] / steps[OFF]["median_ms"], 3)
        steps["frag_kernel_mode_over_default"] = round(steps[ON]["frag_kernel_ms"] / steps[OFF]["frag_kernel_ms"], 3)
        report["c5_step"] = {"shape": f"genomes 0..{C5_GENOMES - 1} of the C5 generator, queries 0..{C5_QUERIES - 1} x the other {C5_GENOMES - 1}", **steps}
        print(json.dumps(report["c5_step"]), flush=True)
    if a.parent_steps:
        runs = [json.loads(Path(f).read_text()) for f in a.parent_steps]
        med = [r["median_ms"] for r in runs]
        spread = round(abs(med[0] - med[1]), 2)
        this = report["c5_step"][OFF]["median_ms"]
        report["default_mode_cost"] = {
            "parent_runs": runs, "parent_medians_ms": med, "parent_spread_ms": spread, "this_median_ms": this,
            "rule": "this_median_ms <= max(parent_medians_ms) + parent_spread_ms",
            "within_parent_spread": bool(this <= max(med) + spread),
            "parent_frag_kernel_ms": [r["frag_kernel_ms"] for r in runs], "this_frag_kernel_ms": report["c5_step"][OFF]["frag_kernel_ms"]}
        print(json.dumps({k: v for k, v in report["default_mode_cost"].items() if k != "parent_runs"}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(report, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
