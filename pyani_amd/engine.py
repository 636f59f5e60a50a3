"""Engine — Python owner of one libpyani_gpu context (one per process and GPU).

Holds genomes resident in HBM (2-bit codes + 1-bit mask) and exposes the TETRA kernels.  numpy arrays are the
only currency across the ctypes boundary; nothing here computes on the CPU.
"""
import ctypes
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


class Engine:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.pg_create(ctypes.byref(h), device)
        if rc == _lib.PG_E_NODEVICE:
            raise _lib.PyaniGpuError(rc, "no HIP device visible: pyani_amd needs an MI355X (there is no CPU fallback)")
        if rc != 0:
            raise _lib.PyaniGpuError(rc, "pg_create failed")
        self._h = h
        self.device = device

    # -- plumbing ---------------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            raise _lib.PyaniGpuError(rc, self.lib.pg_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self.lib.pg_sync(self._h))

    # -- genome store -------------------------------------------------------------------------------------------
    def add_genome(self, seq: np.ndarray, rec_off: Sequence[int]) -> int:
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(rec_off, dtype=np.uint64)
        gid = ctypes.c_int32(-1)
        self._check(self.lib.pg_add_genome(self._h, seq.ctypes.data if seq.size else None, off.ctypes.data,
                                           max(len(off) - 1, 0), ctypes.byref(gid)))
        return gid.value

    def add_fasta(self, path) -> Tuple[int, int, int]:
        """Returns (genome id, total length = sum of record lengths, number of records)."""
        gid, tot, nrec = ctypes.c_int32(-1), ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(self.lib.pg_add_fasta(self._h, str(path).encode(), ctypes.byref(gid), ctypes.byref(tot),
                                          ctypes.byref(nrec)))
        return gid.value, tot.value, nrec.value

    def add_fasta_batch(self, paths, threads: int = 0) -> List[Tuple[int, int, int]]:
        """Multithreaded ingest of many files; returns [(genome id, total length, number of records)] in input order."""
        paths = [str(p).encode() for p in paths]
        n = len(paths)
        arr = (ctypes.c_char_p * n)(*paths)
        ids = np.zeros(n, dtype=np.int32); tot = np.zeros(n, dtype=np.uint64); nrec = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.pg_add_fasta_batch(self._h, ctypes.cast(arr, ctypes.c_void_p), n, int(threads), ids.ctypes.data,
                                                tot.ctypes.data, nrec.ctypes.data))
        return [(int(i), int(t), int(r)) for i, t, r in zip(ids, tot, nrec)]

    def genome_count(self) -> int:
        return self.lib.pg_genome_count(self._h)

    def genome_length(self, gid: int) -> Tuple[int, int]:
        tot, nrec = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(self.lib.pg_genome_length(self._h, gid, ctypes.byref(tot), ctypes.byref(nrec)))
        return tot.value, nrec.value

    def clear_genomes(self):
        self._check(self.lib.pg_clear_genomes(self._h))

    def upload(self):
        self._check(self.lib.pg_upload(self._h))

    def tetra_algorithmic_bytes(self, ids: Optional[Iterable[int]] = None) -> Tuple[int, int]:
        b, n = ctypes.c_uint64(0), ctypes.c_uint64(0)
        if ids is None:
            self._check(self.lib.pg_tetra_algorithmic_bytes(self._h, None, 0, ctypes.byref(b), ctypes.byref(n)))
        else:
            a = np.ascontiguousarray(list(ids), dtype=np.int32)
            self._check(self.lib.pg_tetra_algorithmic_bytes(self._h, a.ctypes.data, len(a), ctypes.byref(b), ctypes.byref(n)))
        return b.value, n.value

    # -- TETRA ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _ids(ids) -> np.ndarray:
        return np.ascontiguousarray(list(ids), dtype=np.int32)

    def tetra_counts(self, ids) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        a = self._ids(ids)
        n = len(a)
        c2, c3, c4 = (np.zeros((n, k), dtype=np.uint64) for k in (16, 64, 256))
        self._check(self.lib.pg_tetra_counts(self._h, a.ctypes.data, n, c2.ctypes.data, c3.ctypes.data, c4.ctypes.data))
        return c2, c3, c4

    def tetra_zscores_from_counts(self, c2, c3, c4) -> Tuple[np.ndarray, np.ndarray]:
        c2, c3, c4 = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, k) for x, k in ((c2, 16), (c3, 64), (c4, 256)))
        n = c4.shape[0]
        z = np.zeros((n, 256), dtype=np.float64)
        present = np.zeros((n, 256), dtype=np.uint8)
        self._check(self.lib.pg_tetra_zscores(self._h, c2.ctypes.data, c3.ctypes.data, c4.ctypes.data, n, z.ctypes.data,
                                              present.ctypes.data))
        return z, present

    def tetra_corr(self, z: np.ndarray, present: np.ndarray) -> np.ndarray:
        z = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 256)
        present = np.ascontiguousarray(present, dtype=np.uint8).reshape(-1, 256)
        n = z.shape[0]
        out = np.zeros((n, n), dtype=np.float64)
        self._check(self.lib.pg_tetra_corr(self._h, z.ctypes.data, present.ctypes.data, n, out.ctypes.data))
        return out

    def tetra_matrix(self, ids, want_corr: bool = True) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """Fused counts -> Z -> Pearson on the device.  Returns (z, present, corr or None)."""
        a = self._ids(ids)
        n = len(a)
        z = np.zeros((n, 256), dtype=np.float64)
        present = np.zeros((n, 256), dtype=np.uint8)
        corr = np.zeros((n, n), dtype=np.float64) if want_corr else None
        self._check(self.lib.pg_tetra_matrix(self._h, a.ctypes.data, n, z.ctypes.data, present.ctypes.data, _ptr(corr)))
        return z, present, corr

    def tetra_matrix_enqueue(self, ids_array: np.ndarray, fetch_z: bool = True):
        self._check(self.lib.pg_tetra_matrix_enqueue(self._h, ids_array.ctypes.data, len(ids_array), int(fetch_z)))

    def tetra_matrix_fetch(self, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        z = np.zeros((n, 256), dtype=np.float64)
        present = np.zeros((n, 256), dtype=np.uint8)
        corr = np.zeros((n, n), dtype=np.float64)
        self._check(self.lib.pg_tetra_matrix_fetch(self._h, n, z.ctypes.data, present.ctypes.data, corr.ctypes.data))
        return z, present, corr

    def tetra_zscores_dev(self, ids, d_z_ptr: int, d_present_ptr: int):
        a = self._ids(ids)
        self._check(self.lib.pg_tetra_zscores_dev(self._h, a.ctypes.data, len(a), d_z_ptr, d_present_ptr))

    def tetra_corr_rows_dev(self, d_z_ptr: int, d_present_ptr: int, n: int, row0: int, nrows: int, d_out_ptr: int):
        self._check(self.lib.pg_tetra_corr_rows_dev(self._h, d_z_ptr, d_present_ptr, n, row0, nrows, d_out_ptr))

    # -- ANIm -------------------------------------------------------------------------------------------------------
    ANIM_DTYPE = np.dtype([("ref_aln_len", "<i8"), ("qry_aln_len", "<i8"), ("sim_errors", "<i8"), ("n_alignments", "<i8"),
                           ("identity", "<f8"), ("status", "<i4"), ("reserved", "<i4")])

    def anim_pairs(self, ref_ids, qry_ids, filter_1to1: bool = True, maxmatch: bool = False) -> np.ndarray:
        """One record per ORDERED pair: ref = nucmer's reference (pyani's query genome), qry = nucmer's query."""
        r, q = self._ids(ref_ids), self._ids(qry_ids)
        if len(r) != len(q):
            raise ValueError("ref_ids and qry_ids must have the same length")
        out = np.zeros(len(r), dtype=self.ANIM_DTYPE)
        self._check(self.lib.pg_anim_pairs(self._h, r.ctypes.data, q.ctypes.data, len(r), int(maxmatch), int(filter_1to1),
                                           out.ctypes.data))
        return out

    def anim_pairs_enqueue(self, ref_ids, qry_ids, filter_1to1: bool = True, maxmatch: bool = False):
        """Non-blocking anim_pairs (pg_anim_pairs_enqueue): returns a ticket at once; at most two calls are in flight per engine, the
        tail of one overlapping the front of the next (pyani's pool keeps its cores busy across job boundaries,
        run_multiprocessing.py:130-144).  Every ticket must be given to anim_pairs_fetch."""
        r, q = self._ids(ref_ids), self._ids(qry_ids)
        if len(r) != len(q):
            raise ValueError("ref_ids and qry_ids must have the same length")
        t = ctypes.c_uint64(0)
        self._check(self.lib.pg_anim_pairs_enqueue(self._h, r.ctypes.data, q.ctypes.data, len(r), int(maxmatch), int(filter_1to1), ctypes.byref(t)))
        return (int(t.value), len(r))

    def anim_pairs_fetch(self, ticket) -> np.ndarray:
        """Waits for the enqueued call and returns its records (the caller's pair order), exactly anim_pairs' result."""
        tid, n = ticket
        out = np.zeros(n, dtype=self.ANIM_DTYPE)
        self._check(self.lib.pg_anim_pairs_fetch(self._h, ctypes.c_uint64(tid), out.ctypes.data, n))
        return out

    def anim_set_workers(self, workers: int = 2) -> None:
        """Host worker threads (streams) sharing one anim_pairs / anib_pairs call: 1 ... 4 (pyani's --workers inside one device)."""
        self._check(self.lib.pg_anim_set_workers(self._h, int(workers)))

    def anim_counters(self, reset: bool = False) -> np.ndarray:
        """The nucmer extender's engine counters since the last reset (include/pyani_gpu.h, pg_anim_counters): uint64[64]."""
        out = np.zeros(64, dtype=np.uint64)
        self._check(self.lib.pg_anim_counters(self._h, out.ctypes.data, int(bool(reset))))
        return out

    def anim_forced_rects(self, ref_id: int, qry_id: int, strand: int, rects) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Development (pg_anim_forced_rects, honoured under PYANI_DEV_KNOBS=1): rectangles (A0, A1, B0, B1) — stream positions, ends
        inclusive, B in strand coordinates — through the extender's forced launches.  Returns (errors, w_used, status) per rectangle:
        w_used -1 = the whole rectangle; status 0 = certified, 2 = corner unreachable / capacity."""
        r = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
        n = len(r)
        errors, w_used, status = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self._check(self.lib.pg_anim_forced_rects(self._h, int(ref_id), int(qry_id), int(strand), n, r.ctypes.data, errors.ctypes.data,
                                                  w_used.ctypes.data, status.ctypes.data))
        return errors, w_used, status

    SEARCH_ENGINES = {"PREPASS": 0, "WALK": 1, "RUNG_256": 2, "RUNG_512": 3, "RUNG_GLOBAL": 4, "LANES": 5}
    SEARCH_FORWARD_ALIGN, SEARCH_BACKWARD_SEARCH, SEARCH_OPTIMAL_BIT = 1, 2, 8

    def anim_searches(self, ref_id: int, qry_id: int, strand: int, engine, searches) -> np.ndarray:
        """Development (pg_anim_searches, honoured under PYANI_DEV_KNOBS=1): trimmed searches (A0, B0, tA, tB, m_o) — stream positions,
        B in strand coordinates — on one of the extender's search engines (a name of SEARCH_ENGINES or its number).  Returns int32[n, 5]:
        endA, endB, errors, reached, held per search (held 0: the engine did not hold the band, the rest is 0)."""
        s = np.ascontiguousarray(searches, dtype=np.int32).reshape(-1, 5)
        out = np.zeros((len(s), 5), dtype=np.int32)
        e = self.SEARCH_ENGINES[engine] if isinstance(engine, str) else int(engine)
        self._check(self.lib.pg_anim_searches(self._h, int(ref_id), int(qry_id), int(strand), e, len(s), s.ctypes.data, out.ctypes.data))
        return out

    def anim_set_batch_budget(self, max_pairs: int, max_matches: int) -> None:
        self._check(self.lib.pg_anim_set_batch_budget(self._h, int(max_pairs), int(max_matches)))

    ALN_DTYPE = np.dtype([("ref_rec", "<i4"), ("qry_rec", "<i4"), ("rs", "<i4"), ("re", "<i4"), ("qs", "<i4"), ("qe", "<i4"),
                          ("errors", "<i4"), ("kept", "<i4")])

    def anim_pair_alignments(self, ref_id: int, qry_id: int) -> np.ndarray:
        """Alignment records of one ordered pair (what nucmer's .delta would hold; kept == 3: survives delta-filter -1)."""
        n = ctypes.c_uint32(0)
        out = np.zeros(4096, dtype=self.ALN_DTYPE)
        self._check(self.lib.pg_anim_pair_alignments(self._h, int(ref_id), int(qry_id), out.ctypes.data, len(out), ctypes.byref(n)))
        if n.value > len(out):
            out = np.zeros(n.value, dtype=self.ALN_DTYPE)
            self._check(self.lib.pg_anim_pair_alignments(self._h, int(ref_id), int(qry_id), out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def anim_alignments_batch(self, ref_ids, qry_ids, maxmatch: bool = False, with_indels: bool = False):
        """Alignment records of MANY ordered pairs in one call (pg_anim_alignments_batch): what pyani's nucmer jobs leave in
        their .delta files for a whole run (anim.py:240-289).  Returns (offsets, records, indel_offsets, indels): pair i owns
        records[offsets[i]:offsets[i + 1]] (ALN_DTYPE; kept == 3: survives delta-filter -1); with_indels=True adds the GPU
        traceback pass: record k's .delta indel offset list is indels[indel_offsets[k]:indel_offsets[k + 1]] (without the
        terminating 0) and the records of a pair come in MUMmer's own output order; else the last two are None."""
        r = np.ascontiguousarray(list(ref_ids), dtype=np.int32)
        q = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        if len(r) != len(q):
            raise ValueError("ref_ids and qry_ids must have the same length")
        offsets = np.zeros(len(r) + 1, dtype=np.uint64)
        n_ind = ctypes.c_uint64(0)
        self._check(self.lib.pg_anim_alignments_batch(self._h, r.ctypes.data, q.ctypes.data, len(r), int(bool(maxmatch)), int(bool(with_indels)),
                                                      offsets.ctypes.data, ctypes.byref(n_ind)))
        recs = np.zeros(int(offsets[-1]), dtype=self.ALN_DTYPE)
        ioff = np.zeros(len(recs) + 1, dtype=np.uint64) if with_indels else None
        ind = np.zeros(int(n_ind.value), dtype=np.int64) if with_indels else None
        self._check(self.lib.pg_anim_alignments_read(self._h, recs.ctypes.data if len(recs) else None, ioff.ctypes.data if with_indels else None,
                                                     ind.ctypes.data if with_indels and len(ind) else None))
        return offsets, recs, ioff, ind

    def anim_reduce(self, pairs, apply_filter: bool = False) -> np.ndarray:
        """pairs: list of per-pair record lists [(rseq, qseq, rs, re, qs, qe, errors), ...] in MUMmer coordinates
        (1-based closed, qs > qe on the reverse strand; rseq/qseq = sequence ordinals within the pair)."""
        offsets = np.zeros(len(pairs) + 1, dtype=np.uint64)
        for k, recs in enumerate(pairs):
            offsets[k + 1] = offsets[k] + len(recs)
        flat = np.array([r for recs in pairs for r in recs], dtype=np.int32).reshape(-1, 7)
        cols = [np.ascontiguousarray(flat[:, c]) for c in range(7)]
        out = np.zeros(len(pairs), dtype=self.ANIM_DTYPE)
        self._check(self.lib.pg_anim_reduce(self._h, len(pairs), offsets.ctypes.data, *(c.ctypes.data for c in cols),
                                            int(apply_filter), out.ctypes.data))
        return out

    def anib_reduce(self, pairs):
        """pairs: list of (n_frags, rows) with rows = [(frag ordinal, length, mismatch, gaps, qlen, pident), ...] in
        file order.  Returns (aln_length int64[], sim_errors int64[], mean pident float64[])."""
        n = len(pairs)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        nfr = np.zeros(max(n, 1), dtype=np.uint32)
        for k, (nf, rows) in enumerate(pairs):
            offsets[k + 1] = offsets[k] + len(rows)
            nfr[k] = nf
        flat = [r for _, rows in pairs for r in rows]
        ints = np.array([r[:5] for r in flat], dtype=np.int32).reshape(-1, 5)
        cols = [np.ascontiguousarray(ints[:, c]) for c in range(5)]
        pid = np.ascontiguousarray([r[5] for r in flat], dtype=np.float64)
        aln, err, out = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
        self._check(self.lib.pg_anib_reduce(self._h, n, offsets.ctypes.data, nfr.ctypes.data, cols[0].ctypes.data,
                                            cols[1].ctypes.data, cols[2].ctypes.data, cols[3].ctypes.data, cols[4].ctypes.data,
                                            pid.ctypes.data, aln.ctypes.data, err.ctypes.data, out.ctypes.data))
        return aln, err, out

    # -- ANIb fragment mode ---------------------------------------------------------------------------------------
    ANIB_DTYPE = np.dtype([("aln_length", "<i8"), ("sim_errors", "<i8"), ("pid", "<f8"), ("n_frags", "<i4"), ("n_kept", "<i4"),
                           ("status", "<i4"), ("reserved", "<i4")])
    ANIB_ROW_DTYPE = np.dtype([("frag", "<i4"), ("length", "<i4"), ("mismatch", "<i4"), ("gaps", "<i4"), ("nident", "<i4"),
                               ("qlen", "<i4"), ("qstart", "<i4"), ("qend", "<i4"), ("sstart", "<i4"), ("send", "<i4"), ("srec", "<i4"),
                               ("score", "<i4")])

    def anib_pairs(self, qry_ids, sbj_ids, fragsize: int = 1020) -> np.ndarray:
        """One record per ORDERED pair: the fragments of genome qry against genome sbj (pyani's blastn job + parse_blast_tab)."""
        q, s = self._ids(qry_ids), self._ids(sbj_ids)
        if len(q) != len(s):
            raise ValueError("qry_ids and sbj_ids must have the same length")
        out = np.zeros(len(q), dtype=self.ANIB_DTYPE)
        self._check(self.lib.pg_anib_pairs(self._h, q.ctypes.data, s.ctypes.data, len(q), int(fragsize), out.ctypes.data))
        return out

    def anib_pair_rows(self, qry_id: int, sbj_id: int, fragsize: int = 1020) -> np.ndarray:
        """The BLAST-shaped table of one ordered pair (<= 4 rows per fragment, best score first)."""
        n = ctypes.c_uint32(0)
        nfr, _ = self.genome_length(qry_id)
        out = np.zeros(4 * (nfr // max(1, fragsize) + 4096), dtype=self.ANIB_ROW_DTYPE)
        self._check(self.lib.pg_anib_pair_rows(self._h, int(qry_id), int(sbj_id), int(fragsize), out.ctypes.data, len(out), ctypes.byref(n)))
        if n.value > len(out):
            out = np.zeros(n.value, dtype=self.ANIB_ROW_DTYPE)
            self._check(self.lib.pg_anib_pair_rows(self._h, int(qry_id), int(sbj_id), int(fragsize), out.ctypes.data, len(out), ctypes.byref(n)))
        return out[:n.value].copy()

    def anib_rows_batch(self, qry_ids, sbj_ids, fragsize: int = 1020) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The tables of MANY ordered pairs in one call (pg_anib_rows_batch): what pyani's blastn jobs leave in their .blast_tab files
        for a whole run.  Returns (results, offsets, rows): results[i] is anib_pairs' record of pair i (ANIB_DTYPE), and pair i owns
        rows[offsets[i]:offsets[i + 1]] (ANIB_ROW_DTYPE), the rows anib_pair_rows gives for it, in the caller's pair order.  Every
        launch packs its rows on the device, so only live rows come back.  A pair with status PG_E_CAPACITY owns no rows."""
        q, s = self._ids(qry_ids), self._ids(sbj_ids)
        if len(q) != len(s):
            raise ValueError("qry_ids and sbj_ids must have the same length")
        out = np.zeros(len(q), dtype=self.ANIB_DTYPE)
        offsets = np.zeros(len(q) + 1, dtype=np.uint64)
        self._check(self.lib.pg_anib_rows_batch(self._h, q.ctypes.data, s.ctypes.data, len(q), int(fragsize), out.ctypes.data,
                                                offsets.ctypes.data))
        return out, offsets, self.anib_rows_read(int(offsets[-1]))

    def anib_rows_read(self, n_rows: int) -> np.ndarray:
        """The rows of the latest anib_rows_batch on this engine (pg_anib_rows_read); n_rows = its offsets[-1].  PyaniGpuError
        (PG_E_ARG) when there has been none."""
        rows = np.zeros(int(n_rows), dtype=self.ANIB_ROW_DTYPE)
        self._check(self.lib.pg_anib_rows_read(self._h, rows.ctypes.data if len(rows) else None))
        return rows

    def anib_set_search(self, mode: str) -> None:
        """Which diagonals fragment mode takes a candidate's initial HSPs from (pg_anib_set_search): "seeds" (the default: the search's
        own seed diagonals) or "all_diagonals" (opt-in: every diagonal of the candidate's band, as blastn does; slower).  Holds for the
        anib_* calls that start after it.  ValueError for any other name."""
        code = _lib.anib_search_code(mode)
        self._check(self.lib.pg_anib_set_search(self._h, code))

    @property
    def anib_search(self) -> str:
        """The search mode the next anib_* call will use (pg_anib_get_search)."""
        m = ctypes.c_uint32(0)
        self._check(self.lib.pg_anib_get_search(self._h, ctypes.byref(m)))
        return {v: k for k, v in _lib.ANIB_SEARCH_MODES.items()}[m.value]

    # -- measurement ----------------------------------------------------------------------------------------------
    # -- sketch mode (fastANI-shaped estimate; never mixed into the exact results) ----------------------------------------------
    SKETCH_DTYPE = np.dtype([("ani", "<f8"), ("matches", "<i4"), ("fragments", "<i4"), ("status", "<i4"), ("reserved", "<i4")])

    SKETCH_FRAGMENT_DTYPE = np.dtype([("window", "<i4"), ("bin", "<i4"), ("hits", "<u4"), ("n", "<u4"), ("identity", "<f8"), ("kept", "<i4"),
                                      ("reserved", "<i4")])

    def sketch_pairs(self, qry_ids, ref_ids, frag_len: int = 3000, scale: int = 16, min_fraction: float = 0.2, kmer: int = 16,
                     mapping: str = "anywhere") -> np.ndarray:
        """pg_sketch_pairs_k: one record per ORDERED pair (query fragmented, reference as a k-mer set): ani (a fraction), matches,
        fragments, status (0 / 1 = fewer than min_fraction of the fragments matched: fastANI writes no line then).  kmer: 8 ... 16.
        mapping="window" (pg_sketch_pairs_mapped, opt-in): a fragment's hits must lie inside one window of two frag_len bins of the
        reference and a reference bin keeps one fragment, as fastANI's mapping does; any other name: ValueError."""
        mapping = _lib.sketch_mapping(mapping)
        q, r = self._ids(qry_ids), self._ids(ref_ids)
        if len(q) != len(r):
            raise ValueError("qry_ids and ref_ids must have the same length")
        out = np.zeros(len(q), dtype=self.SKETCH_DTYPE)
        entry = self.lib.pg_sketch_pairs_mapped if mapping == "window" else self.lib.pg_sketch_pairs_k
        self._check(entry(self._h, q.ctypes.data, r.ctypes.data, len(q), int(kmer), int(frag_len), int(scale), float(min_fraction), out.ctypes.data))
        return out

    def sketch_pair_fragments(self, qry_id: int, ref_id: int, frag_len: int = 3000, scale: int = 16, kmer: int = 16) -> np.ndarray:
        """pg_sketch_pair_fragments: where every fragment of the query mapped under mapping="window" — one SKETCH_FRAGMENT_DTYPE record
        per fragment in fragment order: window, bin (-1: no hit), hits, n, identity (0 when hits < 2), kept (1: counted in the ANI)."""
        n = ctypes.c_uint64(0)
        out = np.zeros(0, dtype=self.SKETCH_FRAGMENT_DTYPE)
        for _ in range(2):      # the count first, then the records
            self._check(self.lib.pg_sketch_pair_fragments(self._h, int(qry_id), int(ref_id), int(kmer), int(frag_len), int(scale),
                                                          out.ctypes.data if len(out) else None, len(out), ctypes.byref(n)))
            if n.value <= len(out):
                break
            out = np.zeros(n.value, dtype=self.SKETCH_FRAGMENT_DTYPE)
        return out[:n.value]

    def sketch_map_last_ms(self) -> Tuple[float, float]:
        """pg_sketch_map_last_ms: (index and grouping build, mapping kernel) milliseconds of the latest mapping="window" call."""
        out = (ctypes.c_double * 2)()
        self._check(self.lib.pg_sketch_map_last_ms(self._h, ctypes.addressof(out)))
        return float(out[0]), float(out[1])

    # -- screen: all-vs-all matrix of shared sampled k-mers (pyani_amd.screen drives these; an estimate for triage) -----------------
    def screen_matrix(self, ids, kmer: int = 16, scale: int = 256, part: int = 0, n_parts: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """pg_screen_matrix: (sizes uint32[n], shared uint32[n, n]) of the genomes in the order given — sizes[a] = the distinct sampled
        canonical k-mers of genome a, shared[a, b] = how many of them genome b holds too (symmetric, the diagonal = sizes).  part /
        n_parts: only the k-mers of that share of the 4096 slice bins; the parts' results add up to the whole, exactly."""
        a = self._ids(ids)
        n = len(a)
        sizes = np.zeros(n, dtype=np.uint32)
        shared = np.zeros((n, n), dtype=np.uint32) if n <= 8192 else np.zeros((0, 0), dtype=np.uint32)      # (beyond: refused before anything is read)
        self._check(self.lib.pg_screen_matrix(self._h, a.ctypes.data if n else None, n, int(kmer), int(scale), int(part), int(n_parts),
                                              sizes.ctypes.data if n else None, shared.ctypes.data if shared.size else None))
        return sizes, shared

    def screen_set_budget(self, max_keys: int = 0) -> None:
        """pg_screen_set_budget: the (k-mer, genome) keys one slice of a screen_matrix call may hold; 0 = the default (2^28)."""
        self._check(self.lib.pg_screen_set_budget(self._h, int(max_keys)))

    def screen_last(self) -> dict:
        """pg_screen_last: counts and stage milliseconds of the latest screen_matrix on this engine."""
        c = (ctypes.c_uint64 * 5)()
        ms = (ctypes.c_double * 3)()
        self._check(self.lib.pg_screen_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"keys": int(c[0]), "distinct": int(c[1]), "groups": int(c[2]), "pair_increments": int(c[3]), "slices": int(c[4]),
                "scan_ms": float(ms[0]), "sort_group_ms": float(ms[1]), "count_ms": float(ms[2])}

    # the selection: one matrix resident on the context, the kept pairs packed on the device
    def screen_hold(self, ids, kmer: int = 16, scale: int = 256, part: int = 0, n_parts: int = 1) -> np.ndarray:
        """pg_screen_hold: screen_matrix without the n^2 read-back — the matrix stays on the device for screen_select; returns sizes."""
        a = self._ids(ids)
        n = len(a)
        sizes = np.zeros(n, dtype=np.uint32)
        self._check(self.lib.pg_screen_hold(self._h, a.ctypes.data if n else None, n, int(kmer), int(scale), int(part), int(n_parts),
                                            sizes.ctypes.data if n else None))
        self._screen_n = n      # (only a call that succeeded leaves a matrix: its size is the one screen_fetch may rely on)
        return sizes

    def screen_load(self, shared) -> None:
        """pg_screen_load: the caller's n x n matrix (uint32; any content) becomes the resident one."""
        m = np.ascontiguousarray(shared, dtype=np.uint32)
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise ValueError(f"a square matrix is needed, not shape {m.shape}")
        self._check(self.lib.pg_screen_load(self._h, m.ctypes.data if m.size else None, m.shape[0]))
        self._screen_n = m.shape[0]

    def screen_select(self, need) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_select + pg_screen_select_read: (a int32[m], b int32[m], shared uint32[m]) of the cells a != b of the resident matrix
        with shared[a][b] >= min(need[a], need[b]), row-major (the order of np.nonzero).  need: uint32[n], n = the resident matrix's."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_select(self._h, t.ctypes.data if len(t) else None, len(t), ctypes.byref(m)))
        a, b, s = np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.uint32)
        self._check(self.lib.pg_screen_select_read(self._h, *(x.ctypes.data if m.value else None for x in (a, b, s))))
        return a, b, s

    def screen_fetch(self) -> np.ndarray:
        """pg_screen_fetch: the resident matrix, uint32[n, n]."""
        n = getattr(self, "_screen_n", 0)      # (the library refuses before it writes when nothing is resident: then n is not looked at)
        out = np.zeros((n, n), dtype=np.uint32)
        self._check(self.lib.pg_screen_fetch(self._h, out.ctypes.data if out.size else None))
        return out

    def screen_release(self) -> None:
        self._check(self.lib.pg_screen_release(self._h))

    def screen_candidates(self, ids, options, labels=None, path: str = "auto"):
        """The pairs of the resident genomes `ids` worth an exact comparison (pyani_amd.screen.ScreenedPairs; options: a ScreenOptions or
        a bare identity threshold).  path "dense": hold -> identity_thresholds -> select -> release, at most 8192 genomes; "index":
        screen_index -> identity_thresholds -> screen_index_select -> release, up to 2^20 genomes, the matrix formed a band at a time
        (DESIGN.md §16.2); "auto": dense up to screen.DENSE_MAX_GENOMES, the index beyond.  Both paths give the same ScreenedPairs: equal,
        in content and order, to screen_genomes(...).candidate_pairs(min_identity, min_shared) without the matrix ever leaving the device."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if screen.resolve_path(path, len(ids)) == "index":
            return screen.index_candidates_on([self], lambda fn: [fn(self, 0)], ids, options, labels)
        return screen.candidates_on(self, lambda: self.screen_hold(ids, options.kmer, options.scale), ids, options, labels)

    # the index: the grouped k-mers resident on the context, the matrix counted and selected a band of rows at a time
    def screen_index(self, ids, kmer: int = 16, scale: int = 256) -> np.ndarray:
        """pg_screen_index: builds the resident k-mer index of the genomes in the order given (up to 2^20) and returns sizes uint32[n]."""
        a = self._ids(ids)
        n = len(a)
        sizes = np.zeros(n if n <= (1 << 20) else 0, dtype=np.uint32)      # (beyond: refused before anything is read)
        self._check(self.lib.pg_screen_index(self._h, a.ctypes.data if n else None, n, int(kmer), int(scale), sizes.ctypes.data if sizes.size else None))
        self._index_n = n      # (only a call that succeeded leaves an index: its size is the one screen_index_band may rely on)
        return sizes

    def screen_set_band(self, rows: int = 0) -> None:
        """pg_screen_set_band: the matrix rows of one band of the index calls, at most 8192; 0 = the default (screen.default_band_rows)."""
        self._check(self.lib.pg_screen_set_band(self._h, int(rows)))
        self._band_rows = int(rows)

    def screen_index_select(self, need, band_first: int = 0, band_step: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_index_select + pg_screen_index_read: screen_select's triples of the bands band_first, band_first + band_step, ...
        of the resident index, row-major."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_index_select(self._h, t.ctypes.data if len(t) else None, len(t), int(band_first), int(band_step), ctypes.byref(m)))
        a, b, s = np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.uint32)
        self._check(self.lib.pg_screen_index_read(self._h, *(x.ctypes.data if m.value else None for x in (a, b, s))))
        return a, b, s

    def screen_index_band(self, band: int) -> np.ndarray:
        """pg_screen_index_band: the finished band `band` of the resident index, uint32[rows of the band, n]: those rows of screen_matrix."""
        from . import screen
        n = getattr(self, "_index_n", 0)      # (the library refuses before it writes when there is no index or no such band)
        ranges = screen.band_ranges(n, getattr(self, "_band_rows", 0))
        r0, r1 = ranges[band] if 0 <= int(band) < len(ranges) else (0, 0)
        out = np.zeros((r1 - r0, n), dtype=np.uint32)
        self._check(self.lib.pg_screen_index_band(self._h, int(band), out.ctypes.data if out.size else None))
        return out

    def screen_index_last(self) -> dict:
        """pg_screen_index_last: counts and stage milliseconds of the latest screen_index and of the latest screen_index_select."""
        c = (ctypes.c_uint64 * 7)()
        ms = (ctypes.c_double * 4)()
        self._check(self.lib.pg_screen_index_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"keys": int(c[0]), "distinct": int(c[1]), "entries": int(c[2]), "groups": int(c[3]), "slices": int(c[4]), "bands": int(c[5]),
                "pair_increments": int(c[6]), "scan_ms": float(ms[0]), "sort_group_ms": float(ms[1]), "count_ms": float(ms[2]), "select_ms": float(ms[3])}

    def screen_index_release(self) -> None:
        self._check(self.lib.pg_screen_index_release(self._h))

    # the components: which genomes belong together, a forest resident on the context
    def _screen_components_read(self, n: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        root, entries, weight = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        self._check(self.lib.pg_screen_components_read(self._h, root.ctypes.data, entries.ctypes.data, weight.ctypes.data))
        return root, entries, weight

    def screen_components(self, a, b, shared=None, n: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_components + pg_screen_components_read: (root int32[n], entries uint64[n], weight uint64[n]) of the list of entries
        (a[e], b[e], shared[e]) over n nodes, as pyani_amd.screen.components_of_pairs states them; shared=None counts 1 everywhere.  The
        number of components is screen_components_last()["components"]."""
        x = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        y = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
        s = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32).reshape(-1)
        if len(x) != len(y) or (s is not None and len(s) != len(x)):
            raise ValueError("a, b and shared must have the same length")
        m = len(x)
        c = ctypes.c_uint32(0)
        self._check(self.lib.pg_screen_components(self._h, x.ctypes.data if m else None, y.ctypes.data if m else None,
                                                  s.ctypes.data if s is not None and m else None, m, int(n), ctypes.byref(c)))
        return self._screen_components_read(int(n))

    def screen_index_components(self, need, band_first: int = 0, band_step: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
        """pg_screen_index_components + pg_screen_components_read: (root, entries, weight, n_pairs) of the kept cells of the bands
        band_first, band_first + band_step, ... of the resident index — screen_components of the list screen_index_select would return,
        n_pairs its length — without a pair leaving the device."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        c, m = ctypes.c_uint32(0), ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_index_components(self._h, t.ctypes.data if len(t) else None, len(t), int(band_first), int(band_step),
                                                        ctypes.byref(c), ctypes.byref(m)))
        return (*self._screen_components_read(len(t)), int(m.value))

    def screen_components_last(self) -> dict:
        """pg_screen_components_last: counts and stage milliseconds of the resident components (all 0 when there are none)."""
        c = (ctypes.c_uint64 * 4)()
        ms = (ctypes.c_double * 3)()
        self._check(self.lib.pg_screen_components_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "entries": int(c[1]), "ignored": int(c[2]), "components": int(c[3]),
                "select_ms": float(ms[0]), "hook_ms": float(ms[1]), "flatten_ms": float(ms[2])}

    def screen_components_release(self) -> None:
        self._check(self.lib.pg_screen_components_release(self._h))

    def screen_components_of(self, ids, options, labels=None, path: str = "auto"):
        """The connected components of the pairs the screen keeps among the resident genomes `ids` (pyani_amd.screen.ScreenComponents).
        path "dense": screen_candidates, then the list entry (the kept pairs are read back once); "index": screen_index ->
        identity_thresholds -> screen_index_components -> release, on errors too — no pair is read back; "auto" as screen_candidates."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if screen.resolve_path(path, len(ids)) == "index":
            return screen.index_components_on([self], lambda fn: [fn(self, 0)], ids, options, labels)
        try:
            return self.screen_candidates(ids, options, labels, path="dense").components(engine=self)
        finally:
            self.screen_components_release()

    # the representatives: one genome per cluster by the greedy rule, rep and via resident on the context
    def _screen_representatives_read(self, n: int) -> Tuple[np.ndarray, np.ndarray]:
        rep, via = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        self._check(self.lib.pg_screen_representatives_read(self._h, rep.ctypes.data, via.ctypes.data))
        return rep, via

    def screen_representatives(self, a, b, weight=None, n: int = 0, score=None) -> Tuple[np.ndarray, np.ndarray]:
        """pg_screen_representatives + pg_screen_representatives_read: (rep int32[n], via uint32[n]) of the list of entries
        (a[e], b[e], weight[e]) over n nodes under the scores score uint64[n], as pyani_amd.screen.representatives_of_pairs states them;
        weight=None weighs every entry 1.  The number of representatives is screen_representatives_last()["representatives"]."""
        x = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        y = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32).reshape(-1)
        if len(x) != len(y) or (w is not None and len(w) != len(x)):
            raise ValueError("a, b and weight must have the same length")
        s = None if score is None else np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
        if s is not None and len(s) != int(n):
            raise ValueError(f"{int(n)} nodes need {int(n)} scores, not {len(s)}")
        m = len(x)
        c = ctypes.c_uint32(0)
        self._check(self.lib.pg_screen_representatives(self._h, x.ctypes.data if m else None, y.ctypes.data if m else None,
                                                       w.ctypes.data if w is not None and m else None, m, int(n),
                                                       s.ctypes.data if s is not None and len(s) else None, ctypes.byref(c)))
        return self._screen_representatives_read(int(n))

    def screen_index_representatives(self, need, score) -> Tuple[np.ndarray, np.ndarray, int]:
        """pg_screen_index_representatives + pg_screen_representatives_read: (rep, via, n_pairs) of the kept cells of ALL bands of the
        resident index — screen_representatives of the list screen_index_select would return, weight = shared, n_pairs its length —
        without a pair leaving the device."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        s = None if score is None else np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
        if s is not None and len(s) != len(t):
            raise ValueError(f"{len(t)} thresholds need {len(t)} scores, not {len(s)}")
        c, m = ctypes.c_uint32(0), ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_index_representatives(self._h, t.ctypes.data if len(t) else None, len(t),
                                                             s.ctypes.data if s is not None and len(s) else None, ctypes.byref(c), ctypes.byref(m)))
        return (*self._screen_representatives_read(len(t)), int(m.value))

    def screen_representatives_last(self) -> dict:
        """pg_screen_representatives_last: counts and stage milliseconds of the resident representatives (all 0 when there are none)."""
        c = (ctypes.c_uint64 * 6)()
        ms = (ctypes.c_double * 4)()
        self._check(self.lib.pg_screen_representatives_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "entries": int(c[1]), "ignored": int(c[2]), "representatives": int(c[3]), "rounds": int(c[4]), "launches": int(c[5]),
                "select_ms": float(ms[0]), "sort_ms": float(ms[1]), "rounds_ms": float(ms[2]), "assign_ms": float(ms[3])}

    def screen_representatives_release(self) -> None:
        self._check(self.lib.pg_screen_representatives_release(self._h))

    def screen_dereplicate(self, ids, options, scores=None, labels=None, path: str = "auto"):
        """The greedy clusters of the pairs the screen keeps among the resident genomes `ids`, weight = shared
        (pyani_amd.screen.ScreenClusters).  scores: one per genome as screen.score_keys takes them, None = the sketch
        sizes.  path "dense": screen_candidates, then the list entry (the kept pairs are read back once); "index": screen_index ->
        identity_thresholds -> screen_index_representatives -> release, on errors too — no pair is read back; "auto" as
        screen_candidates.  Nothing stays resident afterwards."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if scores is not None and len(screen.score_keys(scores)) != len(ids):      # (refused before any work)
            raise ValueError(f"{len(ids)} genomes need {len(ids)} scores")
        if screen.resolve_path(path, len(ids)) == "index":
            labels = screen._labels_for(ids, labels, screen.INDEX_MAX_GENOMES)
            if not ids:
                return screen.clusters_from_nodes(labels, np.zeros(0, np.int32), np.zeros(0, np.uint32), np.zeros(0, np.uint64))
            try:
                sizes = self.screen_index(ids, options.kmer, options.scale)
                need = screen.identity_thresholds(sizes, options.kmer, options.min_identity, options.min_shared)
                score = screen.score_keys(scores, sizes)
                rep, via, _ = self.screen_index_representatives(need, score)
            finally:
                self.screen_index_release()
                self.screen_representatives_release()
            return screen.clusters_from_nodes(labels, rep, via, score)
        try:
            return self.screen_candidates(ids, options, labels, path="dense").representatives(scores, engine=self)
        finally:
            self.screen_representatives_release()

    # the evaluation: how good a partition of the kept pairs is, seven node and seven cluster arrays resident on the context
    def _screen_evaluate_read(self, n: int):
        from . import screen
        nodes = [np.zeros(n, dtype=t) for t in screen._EVALUATE_NODE_TYPES]
        clusters = [np.zeros(n, dtype=t) for t in screen._EVALUATE_CLUSTER_TYPES]
        self._check(self.lib.pg_screen_evaluate_read(self._h, *(x.ctypes.data for x in nodes)))
        self._check(self.lib.pg_screen_evaluate_read_clusters(self._h, *(x.ctypes.data for x in clusters)))
        return tuple(nodes), tuple(clusters)

    @staticmethod
    def _evaluate_inputs(n: int, label, score):
        """label int32[n] and score uint64[n] as the statement checks them (ValueError before the library is called)."""
        from . import screen
        if not 1 <= int(n) <= screen.INDEX_MAX_GENOMES:
            raise ValueError(f"an evaluation is of 1 ... {screen.INDEX_MAX_GENOMES} nodes, not {int(n)}")
        if label is None or score is None:
            raise ValueError("an evaluation needs label= and score=")
        lab = np.ascontiguousarray(screen.check_partition(label, int(n)), dtype=np.int32)
        s = np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
        if len(s) != int(n):
            raise ValueError(f"{int(n)} nodes need {int(n)} scores, not {len(s)}")
        return lab, s

    def screen_evaluate(self, a, b, weight=None, n: int = 0, label=None, score=None):
        """pg_screen_evaluate + pg_screen_evaluate_read + _read_clusters: (the seven node arrays, the seven cluster arrays) of the list of
        entries (a[e], b[e], weight[e]) over n nodes under the partition label int32[n] and the scores score uint64[n], as
        pyani_amd.screen.evaluate_of_pairs states them; weight=None weighs every entry 1.  ValueError as the statement's, before the
        library is called.  The counts are screen_evaluate_last()."""
        from . import screen
        lab, s = self._evaluate_inputs(n, label, score)
        x, y = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32).reshape(-1)
        m = len(x)
        if len(y) != m or (w is not None and len(w) != m):
            raise ValueError("a, b and weight must have the same length")
        if m > screen.EVALUATE_MAX_ENTRIES:
            raise ValueError(f"an evaluation is of at most {screen.EVALUATE_MAX_ENTRIES} entries, not {m}")
        if m and (min(x.min(), y.min()) < 0 or max(x.max(), y.max()) >= int(n)):      # (on the caller's own type: a cast to int32 could hide it)
            raise ValueError(f"an entry names a node outside [0, {int(n)})")
        x, y = np.ascontiguousarray(x, dtype=np.int32), np.ascontiguousarray(y, dtype=np.int32)
        self._check(self.lib.pg_screen_evaluate(self._h, x.ctypes.data if m else None, y.ctypes.data if m else None,
                                                w.ctypes.data if w is not None and m else None, m, int(n), lab.ctypes.data, s.ctypes.data))
        return self._screen_evaluate_read(int(n))

    def screen_index_evaluate(self, need, label, score):
        """pg_screen_index_evaluate + the two reads: (node arrays, cluster arrays, n_pairs) of the kept cells of ALL bands of the
        resident index — screen_evaluate of the list screen_index_select would return, weight = shared, n_pairs its length — without a
        pair leaving the device."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        lab, s = self._evaluate_inputs(len(t), label, score)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_index_evaluate(self._h, t.ctypes.data, len(t), lab.ctypes.data, s.ctypes.data, ctypes.byref(m)))
        return (*self._screen_evaluate_read(len(t)), int(m.value))

    def screen_evaluate_last(self) -> dict:
        """pg_screen_evaluate_last: counts and stage milliseconds of the resident evaluation (all 0 when there is none)."""
        c = (ctypes.c_uint64 * 6)()
        ms = (ctypes.c_double * 4)()
        self._check(self.lib.pg_screen_evaluate_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "entries": int(c[1]), "ignored": int(c[2]), "pairs": int(c[3]), "inside": int(c[4]), "clusters": int(c[5]),
                "select_ms": float(ms[0]), "sort_ms": float(ms[1]), "pair_ms": float(ms[2]), "node_ms": float(ms[3])}

    def screen_evaluate_release(self) -> None:
        self._check(self.lib.pg_screen_evaluate_release(self._h))

    def screen_evaluate_of(self, ids, options, label, scores=None, labels=None, path: str = "auto"):
        """How good the partition `label` of the pairs the screen keeps among the resident genomes `ids` is, weight = shared
        (pyani_amd.screen.ScreenEvaluation).  label: one naming position per genome (screen.check_partition), e.g. the
        rep of screen_dereplicate; scores as screen_dereplicate takes them.  path "dense": screen_candidates, then the list entry (the
        kept pairs are read back once); "index": screen_index -> identity_thresholds -> screen_index_evaluate -> release, on errors too
        — no pair is read back; "auto" as screen_candidates.  Nothing stays resident afterwards."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if scores is not None and len(screen.score_keys(scores)) != len(ids):      # (refused before any work)
            raise ValueError(f"{len(ids)} genomes need {len(ids)} scores")
        label = screen.check_partition(label, len(ids))
        if screen.resolve_path(path, len(ids)) == "index":
            labels = screen._labels_for(ids, labels, screen.INDEX_MAX_GENOMES)
            if not ids:
                return screen.evaluation_from_nodes(labels, label, np.zeros(0, np.uint64), [np.zeros(0)] * 7, [np.zeros(0)] * 7)
            try:
                sizes = self.screen_index(ids, options.kmer, options.scale)
                need = screen.identity_thresholds(sizes, options.kmer, options.min_identity, options.min_shared)
                score = screen.score_keys(scores, sizes)
                nodes, clusters, _ = self.screen_index_evaluate(need, label, score)
            finally:
                self.screen_index_release()
                self.screen_evaluate_release()
            return screen.evaluation_from_nodes(labels, label, score, nodes, clusters)
        try:
            return self.screen_candidates(ids, options, labels, path="dense").evaluate(label, scores, engine=self)
        finally:
            self.screen_evaluate_release()

    # the linkage: species clusters by average / complete linkage inside every component, resident on the context
    def screen_linkage(self, a, b, dist, n: int = 0, score=None, method: str = "average", cutoff: float = 0.05, fill: float = 1.0):
        """pg_screen_linkage + pg_screen_linkage_read + pg_screen_linkage_read_merges: (root, cluster, rep int32[n], merges
        float64[n - components, 4]) of the list of entries (a[e], b[e], dist[e]) over n nodes under the scores score uint64[n], as
        pyani_amd.screen.linkage_of_pairs states them.  ValueError as the statement's, before the library is called.  The number of
        clusters is screen_linkage_last()["clusters"]."""
        from . import screen
        x = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        y = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
        if len(x) != len(y):
            raise ValueError("a, b and dist must have the same length")
        d = screen.check_distances(dist, len(x))
        method, cutoff, fill = screen.check_linkage(method, cutoff, fill)
        s = None if score is None else np.ascontiguousarray(score, dtype=np.uint64).reshape(-1)
        if s is not None and len(s) != int(n):
            raise ValueError(f"{int(n)} nodes need {int(n)} scores, not {len(s)}")
        m = len(x)
        c = ctypes.c_uint32(0)
        self._check(self.lib.pg_screen_linkage(self._h, x.ctypes.data if m else None, y.ctypes.data if m else None, d.ctypes.data if m else None, m, int(n),
                                               s.ctypes.data if s is not None and len(s) else None,
                                               _lib.PG_CLUSTER_AVERAGE if method == "average" else _lib.PG_CLUSTER_COMPLETE, cutoff, fill, ctypes.byref(c)))
        return self._screen_linkage_read(int(n))

    def _screen_linkage_read(self, n: int):
        root, cluster, rep = (np.zeros(n, dtype=np.int32) for _ in range(3))
        self._check(self.lib.pg_screen_linkage_read(self._h, root.ctypes.data, cluster.ctypes.data, rep.ctypes.data))
        rows = n - int(self.screen_linkage_last()["components"])
        merges = np.zeros((rows, 4), dtype=np.float64)
        self._check(self.lib.pg_screen_linkage_read_merges(self._h, merges.ctypes.data if rows else None))
        return root, cluster, rep, merges

    def screen_linkage_set(self, small_limit: Optional[int] = None, work_bytes: int = 0) -> None:
        """pg_screen_linkage_set: components of 2 ... small_limit nodes (0 ... 64; 0: none) run one per wave, the others one per
        workgroup; work_bytes: the working matrices of one batch.  None / 0 restore the defaults.  The results do not depend on either."""
        self._check(self.lib.pg_screen_linkage_set(self._h, _lib.PG_SCREEN_LINKAGE_DEFAULT if small_limit is None else int(small_limit), int(work_bytes)))

    def screen_linkage_last(self) -> dict:
        """pg_screen_linkage_last: counts and stage milliseconds of the resident linkage (all 0 when there is none)."""
        c = (ctypes.c_uint64 * 8)()
        ms = (ctypes.c_double * 5)()
        self._check(self.lib.pg_screen_linkage_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "entries": int(c[1]), "ignored": int(c[2]), "components": int(c[3]), "worked_components": int(c[4]), "largest": int(c[5]),
                "clusters": int(c[6]), "batches": int(c[7]), "group_ms": float(ms[0]), "fill_ms": float(ms[1]), "small_ms": float(ms[2]),
                "large_ms": float(ms[3]), "cut_ms": float(ms[4])}

    def screen_linkage_release(self) -> None:
        self._check(self.lib.pg_screen_linkage_release(self._h))

    # the sweep: the components over a ladder of thresholds in one pass, per-step arrays and snapshots resident on the context
    def _screen_sweep_read(self, n: int, steps: int, n_snapshots: int):
        entries, pair_slots = np.zeros(steps, dtype=np.uint64), np.zeros(steps, dtype=np.uint64)
        components, singletons, largest = (np.zeros(steps, dtype=np.uint32) for _ in range(3))
        self._check(self.lib.pg_screen_sweep_read(self._h, entries.ctypes.data, components.ctypes.data, singletons.ctypes.data, largest.ctypes.data,
                                                  pair_slots.ctypes.data))
        snaps = []
        for k in range(n_snapshots):
            root, e, w = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
            self._check(self.lib.pg_screen_sweep_read_snapshot(self._h, k, root.ctypes.data, e.ctypes.data, w.ctypes.data))
            snaps.append((root, e, w))
        return entries, components, singletons, largest, pair_slots, snaps

    def screen_sweep(self, a, b, shared=None, level=None, n: int = 0, steps: int = 0, snapshots=()):
        """pg_screen_sweep + pg_screen_sweep_read (+ _read_snapshot): (entries uint64[steps], components, singletons, largest
        uint32[steps], pair_slots uint64[steps], [(root, entries, weight) per snapshot]) of the list of entries (a[e], b[e], shared[e])
        with levels level[e] over n nodes, as pyani_amd.screen.sweep_of_pairs states them; shared=None counts 1 everywhere."""
        x = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        y = np.ascontiguousarray(b, dtype=np.int32).reshape(-1)
        s = None if shared is None else np.ascontiguousarray(shared, dtype=np.uint32).reshape(-1)
        lv = np.ascontiguousarray(np.zeros(0, np.uint16) if level is None else level, dtype=np.uint16).reshape(-1)
        if len(x) != len(y) or len(lv) != len(x) or (s is not None and len(s) != len(x)):
            raise ValueError("a, b, shared and level must have the same length")
        snaps = np.ascontiguousarray(list(snapshots), dtype=np.uint32).reshape(-1)
        m = len(x)
        self._check(self.lib.pg_screen_sweep(self._h, x.ctypes.data if m else None, y.ctypes.data if m else None, s.ctypes.data if s is not None and m else None,
                                             lv.ctypes.data if m else None, m, int(n), int(steps), snaps.ctypes.data if len(snaps) else None, len(snaps)))
        return self._screen_sweep_read(int(n), int(steps), len(snaps))

    def screen_index_sweep(self, need, band_first: int = 0, band_step: int = 1, snapshots=()):
        """pg_screen_index_sweep + the reads: screen_sweep's tuple, and n_pairs as its last member, of the kept cells of the bands of the
        resident index under the table need uint32[steps][n] (pyani_amd.screen.sweep_thresholds): selected by row 0, levels found on the
        device — screen_sweep of the list screen_index_select(need[0]) would return with screen.sweep_levels — without a pair leaving
        the device."""
        t = np.ascontiguousarray(need, dtype=np.uint32)
        if t.ndim != 2:
            raise ValueError("a need table is uint32[steps][n]")
        steps, n = t.shape
        snaps = np.ascontiguousarray(list(snapshots), dtype=np.uint32).reshape(-1)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_index_sweep(self._h, t.ctypes.data if t.size else None, n, steps, int(band_first), int(band_step),
                                                   snaps.ctypes.data if len(snaps) else None, len(snaps), ctypes.byref(m)))
        return (*self._screen_sweep_read(n, steps, len(snaps)), int(m.value))

    def screen_sweep_last(self) -> dict:
        """pg_screen_sweep_last: counts and stage milliseconds of the resident sweep (all 0 when there is none)."""
        c = (ctypes.c_uint64 * 6)()
        ms = (ctypes.c_double * 4)()
        self._check(self.lib.pg_screen_sweep_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "steps": int(c[1]), "entries": int(c[2]), "ignored": int(c[3]), "level0": int(c[4]), "buckets": int(c[5]),
                "select_ms": float(ms[0]), "sort_ms": float(ms[1]), "hook_ms": float(ms[2]), "census_ms": float(ms[3])}

    def screen_sweep_release(self) -> None:
        self._check(self.lib.pg_screen_sweep_release(self._h))

    def screen_sweep_of(self, ids, options, identities, labels=None, path: str = "auto", snapshots=()):
        """The components of the pairs the screen keeps among the resident genomes `ids` at EVERY identity of the ladder `identities`
        (strictly ascending, at most 4096; pyani_amd.screen.ScreenSweep).  options.min_identity is IGNORED in favour
        of the ladder: the pairs are those kept at identities[0]; kmer, scale and min_shared are the options'.  path "dense":
        screen_candidates at identities[0], levels on the host, then the list entry (the kept pairs are read back once); "index":
        screen_index -> sweep_thresholds -> screen_index_sweep -> release, on errors too — no pair is read back; "auto" as
        screen_candidates.  Nothing stays resident afterwards.  A single engine: MultiEngine has no sweep."""
        from . import screen
        options = screen.check_options(options)
        t = screen.check_ladder(identities)
        options = options._replace(min_identity=float(t[0]))
        snaps = screen.check_snapshots(snapshots, len(t))
        ids = [int(i) for i in ids]
        if not ids:
            raise ValueError("a sweep needs one genome or more")
        if screen.resolve_path(path, len(ids)) == "index":
            labels = screen._labels_for(ids, labels, screen.INDEX_MAX_GENOMES)
            if len(t) * len(ids) > screen.SWEEP_MAX_TABLE:
                raise ValueError(f"{len(t)} steps x {len(ids)} genomes are more than the 2^28 words of a need table")
            try:
                sizes = self.screen_index(ids, options.kmer, options.scale)
                need = screen.sweep_thresholds(sizes, options.kmer, t, options.min_shared)
                arrays = self.screen_index_sweep(need, snapshots=snaps)[:6]
            finally:
                self.screen_index_release()
                self.screen_sweep_release()
            return screen.sweep_from_arrays(labels, t, arrays, snaps)
        try:
            return self.screen_candidates(ids, options, labels, path="dense").sweep(t, snaps, engine=self)
        finally:
            self.screen_sweep_release()

    # the search: a collection resident as a k-mer index with its keys, new genomes placed against it
    def screen_search_index(self, ids, kmer: int = 16, scale: int = 256, labels=None) -> np.ndarray:
        """pg_screen_search_index: builds the resident SEARCH index of the genomes in the order given (up to 2^20; every distinct k-mer
        with its value, singletons included) and returns sizes uint32[n].  It survives clear_genomes: index the collection, clear the
        store, load the queries.  labels: the db genomes' names for screen_search (default: the ids)."""
        from . import screen
        a = self._ids(ids)
        n = len(a)
        labels = screen.search_labels(a.tolist(), labels, "db")
        sizes = np.zeros(n if n <= (1 << 20) else 0, dtype=np.uint32)      # (beyond: refused before anything is read)
        try:
            self._check(self.lib.pg_screen_search_index(self._h, a.ctypes.data if n else None, n, int(kmer), int(scale), sizes.ctypes.data if sizes.size else None))
        except _lib.PyaniGpuError as err:
            if err.code != _lib.PG_E_ARG:      # refused arguments leave the earlier index; any other failure comes after it was released
                self._search, self._search_q = None, 0
            raise
        self._search = {"n": n, "kmer": int(kmer), "scale": int(scale), "sizes": sizes, "labels": labels}      # (only a call that succeeded leaves an index)
        self._search_q = 0
        return sizes

    def screen_search_index_add(self, ids, labels=None) -> np.ndarray:
        """pg_screen_search_index_add: the genomes `ids` (of the store as it is now) join the resident search index as its last columns,
        without a rebuild: the state is the one screen_search_index over the old list + `ids` would leave.  Returns
        their sizes uint32[m].  The counted rectangle goes; the index's kmer, scale and earlier columns stay.  A collection larger than
        the genome store is indexed in batches: load, index, clear_genomes; load, add, clear_genomes; ...  labels: as for
        screen_search_index."""
        from . import screen
        a = self._ids(ids)
        m = len(a)
        labels = screen.search_labels(a.tolist(), labels, "db")
        info = getattr(self, "_search", None)
        sizes = np.zeros(m if m <= (1 << 20) else 0, dtype=np.uint32)      # (beyond: refused before anything is read)
        # (a failure leaves the old index resident, refused arguments its rectangle too: nothing recorded here changes)
        self._check(self.lib.pg_screen_search_index_add(self._h, a.ctypes.data if m else None, m, sizes.ctypes.data if sizes.size else None))
        if m:
            self._search = dict(info, n=info["n"] + m, sizes=np.concatenate([info["sizes"], sizes]), labels=list(info["labels"]) + labels)
            self._search_q = 0
        return sizes

    def screen_search_add_last(self) -> dict:
        """pg_screen_search_add_last: counts and stage milliseconds of the latest accepted screen_search_index_add (zeros after a build
        or a release)."""
        c = (ctypes.c_uint64 * 6)()
        ms = (ctypes.c_double * 3)()
        self._check(self.lib.pg_screen_search_add_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"genomes": int(c[0]), "keys": int(c[1]), "entries": int(c[2]), "new_kmers": int(c[3]), "matched_kmers": int(c[4]), "adds": int(c[5]),
                "scan_ms": float(ms[0]), "sort_group_ms": float(ms[1]), "merge_ms": float(ms[2])}

    # the search index exported, imported and shrunk
    def screen_search_index_shape(self) -> Tuple[int, int, int, int, int, int, int]:
        """pg_screen_search_index_shape: (n, kmer, scale, D, E, n_slices, keys) of the resident search index."""
        s = (ctypes.c_uint64 * 7)()
        self._check(self.lib.pg_screen_search_index_shape(self._h, ctypes.addressof(s)))
        return tuple(int(x) for x in s)

    def screen_search_index_export(self):
        """pg_screen_search_index_shape + _export: (shape, (kmer uint32[D], start uint64[D + 1], member uint32[E], slice_first
        uint64[n_slices + 1], bin_slice uint32[4096])) of the resident search index.  Nothing resident changes."""
        shape = self.screen_search_index_shape()
        _, _, _, d, e, s, _ = shape
        arrays = (np.zeros(d, dtype=np.uint32), np.zeros(d + 1, dtype=np.uint64), np.zeros(e, dtype=np.uint32), np.zeros(s + 1, dtype=np.uint64),
                  np.zeros(4096, dtype=np.uint32))
        self._check(self.lib.pg_screen_search_index_export(self._h, *(x.ctypes.data if x.size else None for x in arrays)))
        return shape, arrays

    def screen_search_index_import(self, shape, arrays, labels=None) -> np.ndarray:
        """pg_screen_search_index_import: the arrays of an export (or of a file) become the resident search index after the device has
        validated every invariant of a built index (pyani_amd.screen.check_search_index states them); returns the sizes uint32[n] the
        device COMPUTED from the entries.  A refusal (PG_E_ARG) leaves an earlier index, its rectangle and this engine's record as
        they were.  labels: as for screen_search_index (default: the positions)."""
        from . import screen
        shape = tuple(int(x) for x in shape)
        if len(shape) != 7 or min(shape) < 0:
            raise ValueError("the shape of a search index is (n, kmer, scale, D, E, n_slices, keys)")
        n, kmer, scale, d, e, s, _ = shape
        labels = screen.search_labels(list(range(n)), labels, "db")
        kinds = (np.uint32, np.uint64, np.uint32, np.uint64, np.uint32)
        arrays = tuple(np.ascontiguousarray(x, dtype=t).reshape(-1) for x, t in zip(arrays, kinds))
        if tuple(len(x) for x in arrays) != (d, d + 1, e, s + 1, 4096):
            raise ValueError(f"the arrays of a search index of shape {shape} have {d}, {d + 1}, {e}, {s + 1} and 4096 elements, not {[len(x) for x in arrays]}")
        sizes = np.zeros(n if n <= (1 << 20) else 0, dtype=np.uint32)
        c_shape = (ctypes.c_uint64 * 7)(*shape)
        # (a failure leaves the old index resident, a refusal its rectangle too: nothing recorded here changes)
        self._check(self.lib.pg_screen_search_index_import(self._h, ctypes.addressof(c_shape), *(x.ctypes.data if x.size else None for x in arrays),
                                                           sizes.ctypes.data if sizes.size else None))
        self._search = {"n": n, "kmer": kmer, "scale": scale, "sizes": sizes, "labels": labels} if n else None      # (n = 0 leaves no index)
        self._search_q = 0
        return sizes

    def screen_search_index_save(self, path, lengths=None) -> int:
        """The resident search index written to one file (pyani_amd.screen.write_search_index; DESIGN.md §16.7 has the layout) with the
        labels and sizes this engine recorded; lengths: the genomes' lengths, uint64[n] (default zeros).  Returns the file's bytes."""
        from . import screen
        info = getattr(self, "_search", None)
        if not info:
            raise ValueError("no search index on this engine (call screen_search_index first)")
        shape, arrays = self.screen_search_index_export()
        return screen.write_search_index(path, shape, arrays, info["sizes"], info["labels"], lengths)

    def screen_search_index_load(self, path):
        """The search index of a file becomes the resident one: read (np.memmap), imported and validated on the device, and the sizes
        the device computed compared with the stored ones — a mismatch is a ValueError and the index is released.  Returns (sizes,
        labels, lengths).  This engine's record changes after success only."""
        from . import screen
        f = screen.read_search_index(path)
        return self.screen_search_index_adopt(f, str(path))

    def screen_search_index_adopt(self, f, path="the search index file"):
        """screen_search_index_load behind the read: f = pyani_amd.screen.read_search_index(path), for a caller that looks at the header
        before anything is uploaded."""
        sizes = self.screen_search_index_import(f.shape, f.arrays, labels=f.labels)
        if not np.array_equal(sizes, np.asarray(f.sizes, dtype=np.uint32)):
            self.screen_search_index_release()
            raise ValueError(f"{path}: the stored sizes of {int(np.count_nonzero(sizes != f.sizes))} genomes are not the entries the index holds for them")
        return sizes, list(f.labels), np.array(f.lengths, dtype=np.uint64)

    def screen_search_index_remove(self, which) -> None:
        """pg_screen_search_index_remove: the columns `which` — positions (integers) or labels (strings) — leave the resident search
        index without a rebuild: the state is the one screen_search_index over the list without them would leave,
        the later columns move down.  An unknown label, and a label that two columns hold, are ValueErrors.  The counted rectangle
        goes.  Removing every column releases the index.  This engine's record shrinks after success only."""
        info = getattr(self, "_search", None)
        which = list(which)
        cols = []
        for w in which:
            if isinstance(w, str):
                if not info:
                    raise ValueError("no search index on this engine (call screen_search_index first)")
                at = [i for i, x in enumerate(info["labels"]) if x == w]
                if len(at) != 1:
                    raise ValueError(f"the label {w!r} is held by {len(at)} columns of the search index" if at else f"no column of the search index has the label {w!r}")
                cols.append(at[0])
            elif isinstance(w, (bool, float)) or int(w) != w or not 0 <= int(w) < (1 << 32):
                raise ValueError(f"a column to remove is a position or a label, not {w!r}")
            else:
                cols.append(int(w))
        a = np.array(cols, dtype=np.uint32)
        m = len(a)
        self._check(self.lib.pg_screen_search_index_remove(self._h, a.ctypes.data if m else None, m))
        if m:
            keep = np.ones(info["n"], dtype=bool)
            keep[a] = False
            left = int(keep.sum())
            self._search = dict(info, n=left, sizes=info["sizes"][keep], labels=[x for x, k in zip(info["labels"], keep) if k]) if left else None
            self._search_q = 0

    def screen_search_remove_last(self) -> dict:
        """pg_screen_search_remove_last: counts and stage milliseconds of the latest accepted screen_search_index_remove (zeros after a
        build, a load or a release)."""
        c = (ctypes.c_uint64 * 4)()
        ms = (ctypes.c_double * 2)()
        self._check(self.lib.pg_screen_search_remove_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"genomes": int(c[0]), "entries": int(c[1]), "kmers": int(c[2]), "removes": int(c[3]), "mark_ms": float(ms[0]), "compact_ms": float(ms[1])}

    def screen_search_count(self, query_ids) -> np.ndarray:
        """pg_screen_search_count: the rectangle of the resident genomes `query_ids` (at most the band's rows: screen_set_band) against the
        search index stays on the device; returns the queries' sizes uint32[q]."""
        a = self._ids(query_ids)
        q = len(a)
        sizes = np.zeros(q, dtype=np.uint32)
        self._check(self.lib.pg_screen_search_count(self._h, a.ctypes.data if q else None, q, sizes.ctypes.data if q else None))
        self._search_q = q
        return sizes

    def screen_search_select(self, need_q, need_db) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_search_select + pg_screen_search_read: (a int32[m], b int32[m], shared uint32[m]) of the cells of the resident
        rectangle with hits[a][b] >= min(need_q[a], need_db[b]), row-major (pyani_amd.screen.select_rectangle states it)."""
        tq = np.ascontiguousarray(need_q, dtype=np.uint32).reshape(-1)
        td = np.ascontiguousarray(need_db, dtype=np.uint32).reshape(-1)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_search_select(self._h, tq.ctypes.data if len(tq) else None, len(tq), td.ctypes.data if len(td) else None, len(td),
                                                     ctypes.byref(m)))
        a, b, s = np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.int32), np.zeros(m.value, dtype=np.uint32)
        self._check(self.lib.pg_screen_search_read(self._h, *(x.ctypes.data if m.value else None for x in (a, b, s))))
        return a, b, s

    def screen_search_fetch(self) -> np.ndarray:
        """pg_screen_search_fetch: the resident rectangle, uint32[q, n]."""
        info = getattr(self, "_search", None)      # (the library refuses before it writes when nothing is resident: then the shape is not looked at)
        out = np.zeros((getattr(self, "_search_q", 0), info["n"] if info else 0), dtype=np.uint32)
        self._check(self.lib.pg_screen_search_fetch(self._h, out.ctypes.data if out.size else None))
        return out

    def screen_search_last(self) -> dict:
        """pg_screen_search_last: counts and stage milliseconds of the resident search index, the latest count and the latest selection.
        For an index that was loaded (screen_search_index_import) index_sort_group_ms holds the validation's milliseconds and
        index_scan_ms is 0; `keys` is a historical scan count that a remove does not change."""
        c = (ctypes.c_uint64 * 10)()
        ms = (ctypes.c_double * 7)()
        self._check(self.lib.pg_screen_search_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"keys": int(c[0]), "kmers": int(c[1]), "entries": int(c[2]), "slices": int(c[3]), "query_keys": int(c[4]), "lookups": int(c[5]),
                "matched": int(c[6]), "increments": int(c[7]), "query_slices": int(c[8]), "index_bytes": int(c[9]), "index_scan_ms": float(ms[0]), "index_sort_group_ms": float(ms[1]),
                "scan_ms": float(ms[2]), "sort_group_ms": float(ms[3]), "lookup_ms": float(ms[4]), "count_ms": float(ms[5]), "select_ms": float(ms[6])}

    def screen_search_index_release(self) -> None:
        self._check(self.lib.pg_screen_search_index_release(self._h))
        self._search, self._search_q = None, 0

    # the profile: core, private and marker k-mers of every cluster of a partition, read off the resident search index
    def screen_search_profile(self, label, core: float = 0.95, shell: float = 0.15, marker_min_size: int = 2, thresholds=None):
        """pg_screen_search_profile + the four reads: the pyani_amd.screen.ScreenProfile of the resident search index under the partition
        label int32[n] (screen.check_partition: e.g. the rep of screen_dereplicate over the indexed genomes), as
        pyani_amd.screen.profile_of_index states it.  The thresholds are screen.profile_thresholds(size, core, shell), or thresholds =
        (core_need, shell_need), two integer arrays read at naming nodes.  ValueError as the statement's, before the library is called.
        The index, the counted rectangle, the selection and the gather's state stay as they were; the result stays resident until the
        next profile, screen_search_profile_release or close, and survives clear_genomes.  The counts are screen_search_profile_last()."""
        from . import screen
        info = getattr(self, "_search", None)
        if not info:
            raise ValueError("no search index on this engine (call screen_search_index first)")
        n = info["n"]
        lab = screen.check_partition(label, n)
        if thresholds is None:
            core_need, shell_need = screen.profile_thresholds(np.bincount(lab, minlength=n), core, shell)
        else:
            core_need, shell_need = thresholds
        _, core_need, shell_need = screen.check_profile_thresholds(lab, core_need, shell_need)
        if isinstance(marker_min_size, (bool, float)) or not 1 <= int(marker_min_size) < (1 << 32):
            raise ValueError(f"marker_min_size is an integer >= 1, not {marker_min_size!r}")
        lab32 = np.ascontiguousarray(lab, dtype=np.int32)
        m = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_search_profile(self._h, lab32.ctypes.data, core_need.ctypes.data, shell_need.ctypes.data, n, int(marker_min_size), ctypes.byref(m)))
        genomes, clusters, spectrum, markers = self._screen_search_profile_read(n, int(m.value))
        return screen.profile_from_arrays(info["labels"], lab32, core_need, shell_need, int(marker_min_size), genomes, clusters, spectrum, markers, kmer=info["kmer"])

    def _screen_search_profile_read(self, n: int, m: int):
        from . import screen
        genomes = [np.zeros(n, dtype=t) for t in screen._PROFILE_GENOME_TYPES]
        clusters = [np.zeros(n, dtype=t) for t in screen._PROFILE_CLUSTER_TYPES]
        spectrum = np.zeros(n, dtype=np.uint64)
        markers = [np.zeros(m, dtype=t) for t in screen._PROFILE_MARKER_TYPES]
        self._check(self.lib.pg_screen_search_profile_read(self._h, *(x.ctypes.data for x in genomes)))
        self._check(self.lib.pg_screen_search_profile_read_clusters(self._h, *(x.ctypes.data for x in clusters)))
        self._check(self.lib.pg_screen_search_profile_read_spectrum(self._h, spectrum.ctypes.data))
        self._check(self.lib.pg_screen_search_profile_read_markers(self._h, *(x.ctypes.data if m else None for x in markers)))
        return tuple(genomes), tuple(clusters), spectrum, tuple(markers)

    def screen_search_profile_last(self) -> dict:
        """pg_screen_search_profile_last: counts and stage milliseconds of the resident profile (all 0 when there is none)."""
        c = (ctypes.c_uint64 * 10)()
        ms = (ctypes.c_double * 5)()
        self._check(self.lib.pg_screen_search_profile_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"n": int(c[0]), "clusters": int(c[1]), "kmers": int(c[2]), "entries": int(c[3]), "cells": int(c[4]), "lane_kmers": int(c[5]),
                "wave_kmers": int(c[6]), "sorted_kmers": int(c[7]), "sorted_batches": int(c[8]), "markers": int(c[9]),
                "relabel_ms": float(ms[0]), "lane_ms": float(ms[1]), "wave_ms": float(ms[2]), "sorted_ms": float(ms[3]), "marker_ms": float(ms[4])}

    def screen_search_profile_release(self) -> None:
        self._check(self.lib.pg_screen_search_profile_release(self._h))

    def screen_search_profile_set(self, lane_limit: Optional[int] = None, wave_limit: Optional[int] = None, batch_keys: int = 0) -> None:
        """pg_screen_search_profile_set: k-mers of up to lane_limit holders (0 ... 8) go one per thread, up to wave_limit (0 ... 64) one per
        wave, the others through the sorted tier in batches of at most batch_keys entries (0: the budget of screen_set_budget).  None:
        the default.  The result of a profile does not depend on any of them."""
        default = _lib.PG_SCREEN_PROFILE_DEFAULT
        self._check(self.lib.pg_screen_search_profile_set(self._h, default if lane_limit is None else int(lane_limit), default if wave_limit is None else int(wave_limit),
                                                          int(batch_keys)))

    def screen_search(self, query_ids, options, query_labels=None):
        """The db genomes each of the resident genomes `query_ids` is related to (pyani_amd.screen.SearchHits; options: a ScreenOptions
        with the index's kmer and scale, or a bare identity threshold for an index of the defaults): chunks of band_rows queries are
        counted against the resident search index, given their thresholds and selected on the device.  Exactly the cells (query, db
        genome) that screen_candidates over db + queries would keep.  The index stays resident: many searches per index."""
        from . import screen
        options = screen.check_options(options)
        query_ids = [int(i) for i in query_ids]
        query_labels = screen.search_labels(query_ids, query_labels, "query")
        query_sizes, a, b, shared = screen.search_chunks(self, query_ids, options)
        return screen.SearchHits(query_labels, list(self._search["labels"]), options, query_sizes, self._search["sizes"], a, b, shared)

    # the gather: a query decomposed into the genomes of the resident collection
    def screen_gather_count(self, query_ids, abundance: bool = False):
        """pg_screen_gather_count: screen_search_count that also keeps the matched (query, k-mer) entries resident for
        screen_gather_rows; returns the queries' sizes uint32[q].  select and fetch of the search work on its rectangle as before.
        abundance=True (pg_screen_gather_count_abund): the same count, which also keeps every entry's multiplicity
        for screen_gather_abundance; returns (sizes uint32[q], weight uint64[q]: the queries' sampled occurrences W)."""
        a = self._ids(query_ids)
        q = len(a)
        sizes = np.zeros(q, dtype=np.uint32)
        if abundance:
            weight = np.zeros(q, dtype=np.uint64)
            self._check(self.lib.pg_screen_gather_count_abund(self._h, a.ctypes.data if q else None, q, sizes.ctypes.data if q else None,
                                                              weight.ctypes.data if q else None))
            self._search_q = q
            return sizes, weight
        self._check(self.lib.pg_screen_gather_count(self._h, a.ctypes.data if q else None, q, sizes.ctypes.data if q else None))
        self._search_q = q
        return sizes

    def screen_gather_abundance(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_gather_abund + pg_screen_gather_abund_read, after screen_gather_rows over a count with abundance=True: (sum
        uint64[r], sumsq uint64[r, 2] = (lo, hi) words, median2 uint64[r], min uint32[r], max uint32[r]) of the multiplicities of the
        k-mers each recorded row claimed, in the rows' order (pyani_gpu.h states them)."""
        r = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_gather_abund(self._h, ctypes.byref(r)))
        total, sumsq, median2 = np.zeros(r.value, dtype=np.uint64), np.zeros((r.value, 2), dtype=np.uint64), np.zeros(r.value, dtype=np.uint64)
        low, high = np.zeros(r.value, dtype=np.uint32), np.zeros(r.value, dtype=np.uint32)
        self._check(self.lib.pg_screen_gather_abund_read(self._h, *(x.ctypes.data if r.value else None for x in (total, sumsq, median2, low, high))))
        return total, sumsq, median2, low, high

    def screen_gather_abundance_matched(self) -> np.ndarray:
        """pg_screen_gather_abund_matched: uint64[q], MW = the multiplicities of each query's kept entries, summed."""
        out = np.zeros(getattr(self, "_search_q", 0), dtype=np.uint64)
        self._check(self.lib.pg_screen_gather_abund_matched(self._h, out.ctypes.data if out.size else None))
        return out

    def screen_gather_abundance_last(self) -> dict:
        """pg_screen_gather_abund_last: counts and stage milliseconds of the latest abundance count and the latest abundance pass."""
        c = (ctypes.c_uint64 * 4)()
        ms = (ctypes.c_double * 4)()
        self._check(self.lib.pg_screen_gather_abund_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"attributed": int(c[0]), "unattributed": int(c[1]), "holders_walked": int(c[2]), "rank_table_bytes": int(c[3]),
                "weight_ms": float(ms[0]), "attribute_ms": float(ms[1]), "sort_ms": float(ms[2]), "stats_ms": float(ms[3])}

    def screen_gather_rows(self, need, max_ranks: int = 65536) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """pg_screen_gather + pg_screen_gather_read: (query int32[r], db int32[r], unique uint32[r], total uint32[r]) of the greedy
        decomposition of every counted query, ordered by query, then rank (pyani_gpu.h states the rounds).  need: uint32[q] >= 1."""
        t = np.ascontiguousarray(need, dtype=np.uint32).reshape(-1)
        r = ctypes.c_uint64(0)
        self._check(self.lib.pg_screen_gather(self._h, t.ctypes.data if len(t) else None, len(t), int(max_ranks), ctypes.byref(r)))
        qi, db = np.zeros(r.value, dtype=np.int32), np.zeros(r.value, dtype=np.int32)
        unique, total = np.zeros(r.value, dtype=np.uint32), np.zeros(r.value, dtype=np.uint32)
        self._check(self.lib.pg_screen_gather_read(self._h, *(x.ctypes.data if r.value else None for x in (qi, db, unique, total))))
        return qi, db, unique, total

    def screen_gather_matched(self) -> np.ndarray:
        """pg_screen_gather_matched: uint32[q], the entries the latest gather count kept per query = |S(query) & the union of the db|."""
        out = np.zeros(getattr(self, "_search_q", 0), dtype=np.uint32)
        self._check(self.lib.pg_screen_gather_matched(self._h, out.ctypes.data if out.size else None))
        return out

    def screen_gather_fetch(self) -> np.ndarray:
        """pg_screen_gather_fetch: what the latest gather left of the rectangle, uint32[q, n]."""
        info = getattr(self, "_search", None)
        out = np.zeros((getattr(self, "_search_q", 0), info["n"] if info else 0), dtype=np.uint32)
        self._check(self.lib.pg_screen_gather_fetch(self._h, out.ctypes.data if out.size else None))
        return out

    def screen_gather_last(self) -> dict:
        """pg_screen_gather_last: counts and stage milliseconds of the latest gather count and the latest gather."""
        c = (ctypes.c_uint64 * 5)()
        ms = (ctypes.c_double * 3)()
        self._check(self.lib.pg_screen_gather_last(self._h, ctypes.addressof(c), ctypes.addressof(ms)))
        return {"entries": int(c[0]), "rounds": int(c[1]), "rows": int(c[2]), "claimed": int(c[3]), "decrements": int(c[4]),
                "expand_ms": float(ms[0]), "argmax_decide_ms": float(ms[1]), "claim_ms": float(ms[2])}

    def screen_gather(self, query_ids, options, query_labels=None):
        """What each of the resident genomes `query_ids` is MADE OF (pyani_amd.screen.GatherResult; options: a GatherOptions with the
        index's kmer and scale): chunks of band_rows queries are counted against the resident search index with their entries kept,
        given their thresholds and decomposed on the device.  The index stays resident: many gathers per index."""
        from . import screen
        options = screen.check_gather_options(options)
        query_ids = [int(i) for i in query_ids]
        query_labels = screen.search_labels(query_ids, query_labels, "query")
        query_sizes, matched, qi, db, unique, total, *abund = screen.gather_chunks(self, query_ids, options)
        return screen.GatherResult(query_labels, list(self._search["labels"]), options, query_sizes, self._search["sizes"], qi, db, unique, total, matched, *abund)

    # -- classify: clique sweep over identity thresholds (pyani_amd.classify drives these) -------------------------------------
    def classify_edges(self, identity: np.ndarray, coverage: np.ndarray, id_min: float = 0.8, cov_min: float = 0.5) -> Tuple[int, int]:
        """pg_classify_edges: the edges of build_graph_from_results (pyani_classify.py:90-111) from two n x n float64 matrices in one
        label order; they stay resident for classify_sweep.  Returns (number of edges, size of the reference's node set)."""
        i = np.ascontiguousarray(identity, dtype=np.float64)
        c = np.ascontiguousarray(coverage, dtype=np.float64)
        if i.ndim != 2 or i.shape[0] != i.shape[1] or i.shape != c.shape:
            raise ValueError("identity and coverage must be square matrices of one size")
        ne, nn = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(self.lib.pg_classify_edges(self._h, i.ctypes.data, c.ctypes.data, i.shape[0], float(id_min), float(cov_min),
                                               ctypes.byref(ne), ctypes.byref(nn)))
        self._classify_n = i.shape[0]
        return int(ne.value), int(nn.value)

    def classify_edge_identities(self, n_edges: int) -> np.ndarray:
        """The resident edges' identities, unordered (float64[n_edges])."""
        out = np.zeros(int(n_edges), dtype=np.float64)
        self._check(self.lib.pg_classify_edge_identities(self._h, out.ctypes.data if len(out) else None, len(out)))
        return out

    def classify_sweep(self, theta, labels: bool = False) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
        """pg_classify_sweep over the resident edges: step k sees the edges with identity > theta[k] (theta non-decreasing).  Returns
        (components int32[steps], all-cliques bool[steps], labels int32[steps, n] or None: the smallest member index of every node's
        component, -1 outside the node set)."""
        t = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
        n_sub = np.zeros(len(t), dtype=np.int32)
        comp = np.zeros(len(t), dtype=np.uint8)
        lab = np.zeros((len(t), getattr(self, "_classify_n", 0)), dtype=np.int32) if labels else None
        self._check(self.lib.pg_classify_sweep(self._h, t.ctypes.data, len(t), n_sub.ctypes.data, comp.ctypes.data, _ptr(lab)))
        return n_sub, comp.astype(bool), lab

    def classify_release(self) -> None:
        self._check(self.lib.pg_classify_release(self._h))

    # -- heatmap clustering: distances and linkage (pyani_amd.graphics drives these) ---------------------------------------------
    @staticmethod
    def _cluster_matrix(x) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
            raise ValueError(f"a non-empty two-dimensional matrix is needed, not shape {x.shape}")
        return x

    def cluster_pdist(self, x, columns: bool = False) -> np.ndarray:
        """pg_cluster_pdist: scipy's pdist(x) (columns: pdist(x.T), without a transposed copy), Euclidean, condensed order, bit for bit
        (pyani_graphics/mpl/__init__.py:101, :107).  PyaniGpuError with code PG_E_NONFINITE if any distance is NaN or infinite."""
        x = self._cluster_matrix(x)
        n = x.shape[1] if columns else x.shape[0]
        out = np.zeros(n * (n - 1) // 2, dtype=np.float64)
        self._check(self.lib.pg_cluster_pdist(self._h, x.ctypes.data, x.shape[0], x.shape[1], int(bool(columns)), out.ctypes.data if len(out) else None))
        return out

    def cluster_linkage(self, x, method: int = _lib.PG_CLUSTER_COMPLETE, columns: bool = False) -> np.ndarray:
        """pg_cluster_linkage: the (n - 1) x 4 merge records of the nearest-neighbour chain in MERGE order (not yet scipy's Z: see
        pyani_amd.graphics.merges_to_linkage).  Replaces pdist + linkage of add_dendrogram (pyani_graphics/mpl/__init__.py:100-128)."""
        x = self._cluster_matrix(x)
        n = x.shape[1] if columns else x.shape[0]
        out = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
        self._check(self.lib.pg_cluster_linkage(self._h, x.ctypes.data, x.shape[0], x.shape[1], int(bool(columns)), int(method), out.ctypes.data))
        return out

    def cluster_linkage_batch(self, problems) -> List[Optional[np.ndarray]]:
        """pg_cluster_linkage_batch over [(x, columns, method)]: one linkage launch, a workgroup per problem (the ten clusterings of a
        run, subcmd_plot.py:130-139).  Problems that pass the SAME array object share one upload.  Per problem the merge records, or
        None where a distance was not finite."""
        mats = {}
        arr = (_lib.ClusterProblem * len(problems))()
        outs = []
        for k, (x, columns, method) in enumerate(problems):
            if id(x) not in mats:
                mats[id(x)] = self._cluster_matrix(x)
            m = mats[id(x)]
            n = m.shape[1] if columns else m.shape[0]
            out = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
            outs.append(out)
            arr[k].x, arr[k].rows, arr[k].cols = m.ctypes.data, m.shape[0], m.shape[1]
            arr[k].columns, arr[k].method, arr[k].merges = int(bool(columns)), int(method), out.ctypes.data
        self._check(self.lib.pg_cluster_linkage_batch(self._h, ctypes.cast(arr, ctypes.c_void_p), len(problems)))
        return [None if arr[k].status == _lib.PG_E_NONFINITE else outs[k] for k in range(len(problems))]

    # -- neighbour-joining tree of a distance matrix (pyani_amd.tree drives these) -------------------------------------------------
    def tree_nj(self, d) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """pg_tree_nj: (joins (n - 3) x 2 int32, lengths (n - 3) x 2, last 3 int32, last_lengths 3) of the n x n distance matrix d,
        EQUAL to pyani_amd.tree.nj_of_matrix bit for bit.  PyaniGpuError with code PG_E_ARG for n outside 3 ... 8192, an asymmetric
        cell or a non-zero diagonal, PG_E_NONFINITE for a NaN or infinite cell or an overflow."""
        d = np.ascontiguousarray(d, dtype=np.float64)
        if d.ndim != 2 or d.shape[0] != d.shape[1]:
            raise ValueError(f"a square matrix is needed, not shape {d.shape}")
        n = d.shape[0]
        joins, lengths = np.zeros((max(n - 3, 0), 2), dtype=np.int32), np.zeros((max(n - 3, 0), 2), dtype=np.float64)
        last, last_lengths = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.float64)
        self._check(self.lib.pg_tree_nj(self._h, d.ctypes.data if d.size else None, n, joins.ctypes.data if n > 3 else None,
                                        lengths.ctypes.data if n > 3 else None, last.ctypes.data, last_lengths.ctypes.data))
        return joins, lengths, last, last_lengths

    def tree_nj_set(self, tail_limit: int = 512) -> None:
        """pg_tree_nj_set: from tail_limit live nodes down one workgroup runs every remaining step (3 ... 1024; 3 = every step wide).
        The result does not depend on it."""
        if not 0 <= int(tail_limit) <= 0xFFFFFFFF:
            raise ValueError(f"tail_limit must be 3 ... 1024, not {tail_limit}")
        self._check(self.lib.pg_tree_nj_set(self._h, int(tail_limit)))

    def tree_nj_last(self) -> Tuple[Dict[str, int], Dict[str, float]]:
        """pg_tree_nj_last: the latest tree_nj's counts (n, wide_steps, tail_steps, launches, cells_scanned) and its stage
        milliseconds (validate_ms, wide_ms, tail_ms; zeros unless profile_enable() is on)."""
        counts, ms = (ctypes.c_uint64 * 5)(), (ctypes.c_double * 3)()
        self._check(self.lib.pg_tree_nj_last(self._h, ctypes.addressof(counts), ctypes.addressof(ms)))
        return (dict(zip(("n", "wide_steps", "tail_steps", "launches", "cells_scanned"), (int(c) for c in counts))),
                dict(zip(("validate_ms", "wide_ms", "tail_ms"), (float(v) for v in ms))))

    # -- distribution plots: histogram and kernel density estimate (pyani_amd.graphics drives these) ------------------------------
    def dist_load(self, x) -> Tuple[float, float, int, int]:
        """pg_dist_load: uploads the values (any shape, taken in C order) and keeps them resident for dist_hist / dist_kde.  Returns
        (min, max, NaN cells, +-inf cells); min and max are over the non-NaN values (pyani_graphics/mpl/__init__.py:149-150)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        st = _lib.DistStats()
        self._check(self.lib.pg_dist_load(self._h, x.ctypes.data if len(x) else None, len(x), ctypes.addressof(st)))
        return float(st.min), float(st.max), int(st.n_nan), int(st.n_inf)

    def dist_hist(self, edges) -> np.ndarray:
        """pg_dist_hist over the resident values: np.histogram(values, edges)[0] as int64, exactly (pyani_graphics/mpl/__init__.py:152)."""
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        counts = np.zeros(max(len(e) - 1, 0), dtype=np.uint64)
        self._check(self.lib.pg_dist_hist(self._h, e.ctypes.data, len(counts), counts.ctypes.data if len(counts) else None))
        return counts.astype(np.int64)

    def dist_kde(self, points, bandwidth: float) -> np.ndarray:
        """pg_dist_kde over the resident values: sum_i exp(-((p_j - x_i) / bandwidth)^2 / 2) per point, float64, NOT normalised (the sum
        inside scipy's gaussian_kde.evaluate, pyani_graphics/mpl/__init__.py:154-156)."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        out = np.zeros(len(p), dtype=np.float64)
        self._check(self.lib.pg_dist_kde(self._h, p.ctypes.data if len(p) else None, len(p), float(bandwidth), out.ctypes.data if len(p) else None))
        return out

    def dist_release(self) -> None:
        self._check(self.lib.pg_dist_release(self._h))

    def dist_last_ms(self) -> Tuple[float, float, float]:
        """Kernel milliseconds of the latest dist_load (stats pass), dist_hist and dist_kde; zeros unless profile_enable() is on."""
        out = (ctypes.c_double * 3)()
        self._check(self.lib.pg_dist_last_ms(self._h, ctypes.addressof(out)))
        return out[0], out[1], out[2]

    def profile_enable(self, on: bool = True):
        self._check(self.lib.pg_profile_enable(self._h, int(on)))

    def profile_config(self, kernel_mask: int = 0xFFFFFFFF, every_n: int = 1):
        self._check(self.lib.pg_profile_config(self._h, kernel_mask, every_n))

    def profile_reset(self):
        self._check(self.lib.pg_profile_reset(self._h))

    def profile_get(self, which: int) -> Tuple[float, int]:
        ms, n = ctypes.c_double(0), ctypes.c_uint64(0)
        self._check(self.lib.pg_profile_get(self._h, which, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def kernel_name(self, which: int) -> str:
        return self.lib.pg_kernel_name(which).decode()


_default: List[Optional[Engine]] = [None]


def default_engine() -> Engine:
    """Process-wide engine on LOCAL_RANK's GPU (created on first use)."""
    import os
    if _default[0] is None:
        _default[0] = Engine(int(os.environ.get("LOCAL_RANK", "0")))
    return _default[0]
