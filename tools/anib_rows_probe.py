"""What the batched ANIb tables cost against the loop of single-pair calls they replace ("ANIb tables of a run").

Two sets of ordered pairs:
  synthetic_72   the 72 ordered pairs of nine related ~6 kb genomes (tests/test_anib_rows_batch_gpu.py, chunk test)
  caulobacter_12 the 12 ordered pairs of the four Caulobacter genomes under tests/golden/genomes/caulobacter
For each set: (a) a loop of Engine.anib_pair_rows, one call per pair, and (b) ONE Engine.anib_rows_batch call.  One warm-up of
each, then the median wall time of 5 repeats; the engine is synchronised before every clock reading.  Bytes read back for the
rows: (a) every fragment slot's padded scratch, 4 rows x 48 B + a 4 B count per slot; (b) the live rows x 48 B + a 4 B count per
pair (+ one 4 B total per launch, not counted).  Writes profiles/anib_rows_probe.json (or --out).

    python tools/anib_rows_probe.py [--out FILE] [--repeats 5]
"""
import argparse
import gzip
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _timed(eng, fn, repeats):
    fn()                                   # warm-up: seed lists, word indices, scratch growth
    times = []
    for _ in range(repeats):
        eng.sync()
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, out


def probe_set(eng, name, qs, ss, repeats):
    loop_s, loop_all, tables = _timed(eng, lambda: [eng.anib_pair_rows(q, s) for q, s in zip(qs, ss)], repeats)
    batch_s, batch_all, (res, off, rows) = _timed(eng, lambda: eng.anib_rows_batch(qs, ss), repeats)
    assert [len(t) for t in tables] == np.diff(np.asarray(off, dtype=np.int64)).tolist()
    assert np.concatenate(tables).tobytes() == rows.tobytes() if len(rows) else True
    slots = int(res["n_frags"].astype(np.int64).sum())
    return {"set": name, "pairs": len(qs), "fragment_slots": slots, "rows": int(off[-1]),
            "loop_of_pair_rows_s": loop_s, "rows_batch_s": batch_s, "batch_over_loop": batch_s / loop_s,
            "loop_of_pair_rows_all_s": loop_all, "rows_batch_all_s": batch_all,
            "loop_bytes_read_back": slots * (4 * 48 + 4), "batch_bytes_read_back": int(off[-1]) * 48 + len(qs) * 4}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "anib_rows_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pyani_amd import synth
    from pyani_amd.engine import Engine
    report = {"repeats": args.repeats, "statistic": "median wall seconds after one warm-up, engine synchronised before each clock reading", "sets": []}
    with Engine(0) as eng:
        g = [eng.add_genome(*synth.genome(77, 9, k, 6_000)) for k in range(9)]
        pairs = [(a, b) for a in g for b in g if a != b]
        order = np.random.RandomState(5).permutation(len(pairs))
        report["sets"].append(probe_set(eng, "synthetic_72", [pairs[k][0] for k in order], [pairs[k][1] for k in order], args.repeats))
        eng.clear_genomes()
        with tempfile.TemporaryDirectory() as tmp:
            ids = []
            for gz in sorted((ROOT / "tests" / "golden" / "genomes" / "caulobacter").glob("*.fna.gz")):
                dst = Path(tmp) / gz.name[:-3]
                with gzip.open(gz, "rb") as fi, open(dst, "wb") as fo:
                    shutil.copyfileobj(fi, fo)
                ids.append(eng.add_fasta(dst)[0])
        pairs = [(a, b) for a in ids for b in ids if a != b]
        report["sets"].append(probe_set(eng, "caulobacter_12", [p[0] for p in pairs], [p[1] for p in pairs], args.repeats))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(report, indent=1, sort_keys=True) + "\n")
    for s in report["sets"]:
        print(f"{s['set']}: loop {s['loop_of_pair_rows_s'] * 1e3:.1f} ms, batch {s['rows_batch_s'] * 1e3:.1f} ms (x{s['batch_over_loop']:.3f}); "
              f"read back {s['loop_bytes_read_back']} -> {s['batch_bytes_read_back']} B")


if __name__ == "__main__":
    main()
