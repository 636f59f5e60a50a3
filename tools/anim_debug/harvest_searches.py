#!/usr/bin/env python3
"""Harvest trimmed searches whose band does not fit the 256-diagonal window (the `outgrow` group of tests/search_cases.py).

Constructions do not get there (fifteen tried stayed at <= 102 cells per anti-diagonal against the window's ~125), so the host
statement is run with the emulated wave engines (tools/anim_debug/anim_debug.cpp, ANIM_DIAGWAVE=1) over the synthetic workloads the
project already generates, with ANIM_FALLBACK_LOG=1: every call the window did not hold is logged with its positions.  Each logged
search is then cut out of its two streams with a margin of 300 bases and printed as a case: name, mode, and the two sequences (the query
as stored, i.e. of the forward strand).  Workloads: divergent pairs of one C4 family and of C3's family 3 (pyani_amd.synth, at the
length given), the stress pairs of tests/stress_genomes.py, the tandem genomes of tests/test_seed_passes_gpu.py.

  python tools/anim_debug/harvest_searches.py [--length 1000000] [--jobs 8] [--out DIR] [--only c4_]

Writes DIR/<case>.txt (one line: name strand A0 B0 tA tB m_o, then the reference cut, then the query cut) and prints, per workload,
the number of calls of the 256-diagonal engine looked at and the searches that did not fit (tools/anim_debug/searches then says
whether the 512-diagonal window holds them).  The run behind tests/search_cases.py found none: see the `outgrow` group there."""
import argparse
import os
import random
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
MARGIN = 300


def workloads(L):
    from pyani_amd import synth
    from tests import stress_genomes as sg
    out = []      # (name, [(record strings of the reference), (of the query)])

    def syn(seed, n, g):
        seq, off = synth.genome(seed, n, g, L)
        s = bytes(seq).decode()
        return [s[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]

    # C4 (1000 genomes: 40 ancestors; family k = genomes k, k + 40, k + 80 ...; substitution rates 0.1 ... 15 % by g // 40 % 6): families 0 - 3
    for a, b in ((160, 200), (200, 160), (120, 200), (160, 400), (200, 440), (80, 200), (120, 160), (400, 440), (80, 120), (120, 360), (360, 120), (80, 160),
                 (160, 120), (120, 80), (80, 320), (320, 360), (360, 400), (40, 160), (0, 160), (121, 161), (122, 162), (123, 163)):
        out.append((f"c4_{a}_{b}", syn(20250301, 1000, a), syn(20250301, 1000, b)))
    # C3 (200 genomes: 8 ancestors), family 3: its first four genomes and the two most divergent
    for a, b in ((3, 11), (11, 19), (19, 27), (27, 3), (35, 43), (43, 35), (35, 27)):
        out.append((f"c3_{a}_{b}", syn(20250228, 200, a), syn(20250228, 200, b)))
    for t in range(24):
        ref, qry = sg.make_rearranged_pair(random.Random(3000017 + t))
        out.append((f"stress_rearranged_{t}", ref, qry))
    for t in range(40):
        ref, qry = sg.make_tandem_pair(random.Random(7000001 + t))
        out.append((f"stress_tandem_{t}", [ref], [qry]))
    for t in sg.TWO_STRAND_TRIALS:
        ref, qry = sg.make_two_strand_repeat_pair(random.Random(13000003 + t))
        out.append((f"stress_two_strand_{t}", ref, qry))
    # the tandem genomes of tests/test_seed_passes_gpu.py: 300 kb of a family member + 9000 copies of a 40-base unit, and two relatives
    ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
    fam = [synth.genome(20250702, 4, g, 300_000) for g in range(3)]
    unit = ACGT[np.random.RandomState(5).randint(0, 4, 40)]
    R = bytes(fam[0][0][:300_000]).decode() + bytes(np.tile(unit, 9000)).decode()
    B, C = (bytes(f[0]).decode() for f in fam[1:])
    out += [("tandem_R_B", [R], [B]), ("tandem_B_R", [B], [R]), ("tandem_R_C", [R], [C])]
    fa = [synth.genome(20250701, 4, g, 300_000) for g in range(4)]
    tandem = bytes(np.tile(ACGT[np.random.RandomState(11).randint(0, 4, size=1000)], 600)).decode()
    g0 = bytes(fa[0][0][:150_000]).decode() + tandem
    s1 = bytes(fa[1][0]).decode()
    g1 = s1[:len(s1) // 2] + tandem + s1[len(s1) // 2:]
    out += [("tandem_a_0_1", [g0], [g1]), ("tandem_a_1_0", [g1], [g0])]
    return out


def run_pair(args):
    name, ref, qry, tmp, exe = args
    fr, fq = Path(tmp) / f"{name}_r.fna", Path(tmp) / f"{name}_q.fna"
    for f, recs in ((fr, ref), (fq, qry)):
        f.write_text("".join(f">r{k}\n{s}\n" for k, s in enumerate(recs)))
    env = dict(os.environ, ANIM_DIAGWAVE="1", ANIM_FALLBACK_LOG="1")
    p = subprocess.run([str(exe), str(fr), str(fq)], capture_output=True, text=True, env=env)
    calls = sum(int(m.group(1)) for m in re.finditer(r"diag-wave engines: calls \d+ / (\d+) /", p.stderr))
    logged = [tuple(int(v) for v in m.groups()) for m in re.finditer(
        r"FALLBACK search N \d+ M \d+ strand (\d) start (-?\d+) (-?\d+) target (-?\d+) (-?\d+) m_o (\d+)", p.stderr)]
    # the streams as the host tool lays them out: records joined by one separator (never a clean base)
    return name, p.returncode, calls, logged, "#".join(ref), "#".join(qry)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default="harvest_out")
    ap.add_argument("--only", default="", help="only the workloads whose name starts with this")
    a = ap.parse_args()
    exe = ROOT / "tools" / "anim_debug" / "anim_debug"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(exe) + ".cpp", "-o", str(exe)], check=True)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    total_calls = total_found = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as ex:
        for name, rc, calls, logged, rs, qs in ex.map(run_pair, [(n, r, q, tmp, exe) for n, r, q in workloads(a.length) if n.startswith(a.only)]):
            print(f"{name}: exit {rc}, {calls} calls on the 256-diagonal window, {len(logged)} did not fit", flush=True)
            total_calls += calls
            total_found += len(logged)
            for k, (strand, A0, B0, tA, tB, m_o) in enumerate(logged):
                m_o &= 11      # (SEARCH_BIT is the backward direction itself)
                a_lo, a_hi = max(0, min(A0, tA) - MARGIN), min(len(rs), max(A0, tA) + 1 + MARGIN)
                b_lo, b_hi = max(0, min(B0, tB) - MARGIN), min(len(qs), max(B0, tB) + 1 + MARGIN)
                ca = rs[a_lo:a_hi].replace("#", "N")
                if strand:      # strand positions p of the reverse strand are stored positions len - 1 - p
                    cb = qs[len(qs) - b_hi:len(qs) - b_lo].replace("#", "N")      # as stored: the cut's own reverse strand starts at b_lo
                else:
                    cb = qs[b_lo:b_hi].replace("#", "N")
                (out / f"{name}_{k}.txt").write_text(f"{name}_{k} {strand} {A0 - a_lo} {B0 - b_lo} {tA - a_lo} {tB - b_lo} {m_o}\n{ca}\n{cb}\n")
    print(f"total: {total_calls} calls looked at, {total_found} did not fit the 256-diagonal window")


if __name__ == "__main__":
    main()
