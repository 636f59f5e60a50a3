"""ctypes binding of oracle/libanibcpu.so — the host statement of fragment mode (oracle/anib_cpu.cpp).
TEST / MEASUREMENT INFRASTRUCTURE ONLY."""
import ctypes
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import oracle_build as _obuild  # noqa: E402

ROW_DTYPE = np.dtype([("frag", "<i4"), ("length", "<i4"), ("mismatch", "<i4"), ("gaps", "<i4"), ("nident", "<i4"), ("qlen", "<i4"),
                      ("qstart", "<i4"), ("qend", "<i4"), ("sstart", "<i4"), ("send", "<i4"), ("srec", "<i4"), ("score", "<i4")])


_I32 = "<i4"
FS_DTYPE = np.dtype([(k, _I32) for k in ("frag", "strand", "own_seeds", "word_found", "word_taken", "cands", "lone_weak", "prelims",
                                         "finals", "rows_pre", "rows_post", "listed")])
EXT_DTYPE = np.dtype([(k, _I32) for k in ("frag", "strand", "kind", "recentres", "net", "lo", "hi", "left_low", "left_high", "di", "dj",
                                          "score")])
EXT_KINDS = ("prelim_right", "prelim_left", "weak_right", "weak_left", "right", "left", "left_again", "right_again")


def _library(defines=None):
    return ctypes.CDLL(str(_obuild.build_anib_cpu_variant(defines) if defines else _obuild.build_anib_cpu()))


def anib_cpu_pair_trace(query, subject, fragsize=1020):
    """anib_cpu_pair's rows plus what the statement did on the way: (rows, fs, ext).
    fs: one record per (fragment, strand) — own seeds before the cap, word seeds found / taken, seeds listed, candidates, lone weak
    candidates aligned, preliminary alignments, final alignments, rows that pass the e-value cut, rows in the table.
    ext: one record per extension (kind: index into EXT_KINDS) — re-centrings that moved the band, its offset from where it started at
    the best cell / lowest / highest until then (re-centrings likewise: up to the best cell), whether a live state stood on the band's
    first / last diagonal or was shifted out there at ANY time of the extension (the dying-out after the best cell included), bases
    consumed, best score."""
    lib = _library()
    lib.anib_cpu_pair_trace.restype = ctypes.c_int64
    qs, qo = np.ascontiguousarray(query[0], dtype=np.uint8), np.ascontiguousarray(query[1], dtype=np.uint64)
    ss, so = np.ascontiguousarray(subject[0], dtype=np.uint8), np.ascontiguousarray(subject[1], dtype=np.uint64)
    nfrag = len(qs) // fragsize + len(qo) + 8
    cap, fs_cap, ext_cap = 4 * nfrag, 2 * nfrag, 2 * nfrag * 8 * 14
    out, fs, ext = np.zeros(cap, dtype=ROW_DTYPE), np.zeros(fs_cap, dtype=FS_DTYPE), np.zeros(ext_cap, dtype=EXT_DTYPE)
    counts = np.zeros(2, dtype=np.uint64)
    n = lib.anib_cpu_pair_trace(ctypes.c_void_p(qs.ctypes.data), ctypes.c_void_p(qo.ctypes.data), ctypes.c_uint32(len(qo) - 1),
                                ctypes.c_void_p(ss.ctypes.data), ctypes.c_void_p(so.ctypes.data), ctypes.c_uint32(len(so) - 1),
                                ctypes.c_int32(fragsize), ctypes.c_void_p(out.ctypes.data), ctypes.c_uint64(cap),
                                ctypes.c_void_p(fs.ctypes.data), ctypes.c_uint64(fs_cap), ctypes.c_void_p(ext.ctypes.data),
                                ctypes.c_uint64(ext_cap), ctypes.c_void_p(counts.ctypes.data))
    assert 0 <= n <= cap and counts[0] <= fs_cap and counts[1] <= ext_cap, (n, counts)
    return out[:n], fs[:int(counts[0])], ext[:int(counts[1])]


def anib_cpu_pair(query, subject, fragsize=1020, defines=None):
    """query / subject: (uint8 sequence array, uint64 record offsets).  Rows of the BLAST-shaped table of the ordered pair
    (fragments of `query` against `subject`), best score first within a fragment.
    defines: a list of "NAME=VALUE" strings — the variant of the statement built with them (oracle_build.build_anib_cpu_variant)."""
    lib = _library(defines)
    lib.anib_cpu_pair.restype = ctypes.c_int64
    qs, qo = np.ascontiguousarray(query[0], dtype=np.uint8), np.ascontiguousarray(query[1], dtype=np.uint64)
    ss, so = np.ascontiguousarray(subject[0], dtype=np.uint8), np.ascontiguousarray(subject[1], dtype=np.uint64)
    cap = 4 * (len(qs) // fragsize + len(qo) + 8)
    out = np.zeros(cap, dtype=ROW_DTYPE)
    n = lib.anib_cpu_pair(ctypes.c_void_p(qs.ctypes.data), ctypes.c_void_p(qo.ctypes.data), ctypes.c_uint32(len(qo) - 1),
                          ctypes.c_void_p(ss.ctypes.data), ctypes.c_void_p(so.ctypes.data), ctypes.c_uint32(len(so) - 1),
                          ctypes.c_int32(fragsize), ctypes.c_void_p(out.ctypes.data), ctypes.c_uint64(cap))
    assert 0 <= n <= cap
    return out[:n]


def reduce_rows(rows):
    """parse_blast_tab's arithmetic (pyani/anib.py:641-665) over such rows: (aln_length, sim_errors, mean pident, kept rows).
    pident as BLAST prints it: 3 decimals."""
    aln = err = 0
    pids, kept, seen = [], [], set()
    for r in rows:
        f = int(r["frag"])
        if f in seen:
            continue
        alnlen = int(r["length"]) - int(r["gaps"])
        if alnlen / int(r["qlen"]) > 0.7 and (alnlen - int(r["mismatch"])) / int(r["qlen"]) > 0.3:
            seen.add(f)
            kept.append(r)
            aln += alnlen
            err += int(r["mismatch"]) + int(r["gaps"])
            pids.append(float("%.3f" % (100.0 * int(r["nident"]) / int(r["length"]))))
    return aln, err, (sum(pids) / len(pids) if pids else 0.0), kept
