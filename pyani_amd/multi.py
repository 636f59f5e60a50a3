"""MultiEngine — one process, several GPUs: the in-product answer to pyani's `--workers` (SURVEY.md §8 e).

pyani spreads its nucmer / blastn jobs over `--workers` CPU cores with a multiprocessing pool
(`scripts/subcommands/subcmd_anim.py:392-396` -> `run_multiprocessing.run_dependency_graph(jobs, workers=...)`,
`run_multiprocessing.py:113-152`): independent jobs, handed out as workers fall idle.  Here a "worker" is a GPU: one Engine (one
libpyani_gpu context) per device, every genome resident on every device (1.9 GB for 1000 x 5 Mb of the 288 GB each has), and the
ordered-pair list cut into chunks that the devices PULL from a shared queue — one host thread per device, the ctypes calls release
the GIL — so a device that drew cheap chunks (unrelated pairs cost microseconds, related ones milliseconds: ~60 x apart) simply
comes back for more.  No data-path collective: results are merged on the host in the caller's order.  The multi-process RCCL
path (`pyani_amd/parallel.py`, `bench.py --gpus N`: one process per GPU, one all-gather per step) stays what the driver's scaling
run measures; this class is what `run_anim(..., devices=[...])` and the module functions use.

A chunk keeps a pair and its reverse together (they share their seeding inside one `pg_anim_pairs` call, DESIGN.md §5c "Roles") and
keeps the pairs of one reference genome together (its seed table is built once per call).  Results do not depend on the number of
devices or on which device ran what (tests/test_parallel_multi_gpu.py: two engines on GPU 0 == one).
"""
import threading
from collections import defaultdict
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import _lib
from .engine import Engine


def _chunks_by_hub(a: np.ndarray, b: np.ndarray, target: int) -> List[np.ndarray]:
    """Indices of the pair list grouped so that (x, y) and (y, x) share a chunk and the pairs of one hub genome stay together;
    chunks of about `target` pairs, heaviest first is not knowable, so: in hub order."""
    n = len(a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    # the hub of an unordered pair {lo, hi}: lo when lo + hi is even, hi otherwise — every genome hubs half of its partners
    hub = np.where(((lo + hi) & 1) == 0, lo, hi)
    order = np.argsort(hub, kind="stable")
    bounds = np.flatnonzero(np.diff(hub[order])) + 1
    groups = np.split(order, bounds)
    out, cur, size = [], [], 0
    for g in groups:
        cur.append(g)
        size += len(g)
        if size >= target:
            out.append(np.concatenate(cur)); cur, size = [], 0
    if cur:
        out.append(np.concatenate(cur))
    assert sum(len(c) for c in out) == n
    return out


def _static_parts_by_hub(a: np.ndarray, b: np.ndarray, parts: int) -> List[np.ndarray]:
    """The pair list dealt into `parts` shares, ONE call each: the hub groups of _chunks_by_hub in a fixed scrambled order
    (multiplicative hash of the hub id: related genomes sit next to each other in sorted input lists and at a fixed stride in the
    synthetic sets), dealt round-robin.  Why one big call per device and not a queue of small ones (measured on MI355X, C4,
    profiles/r05_deal_probe.json): a call's kernels each end with their longest item — one forced re-alignment can take 100 ms — so a
    call of 100 hub rows costs 20 ms per row, 25 rows 26 ms, 6 rows 51 ms, 2 rows 72 ms; the dynamic deal of round 4 (chunks down to
    2 rows) ran at 48 % of the plain rate, while the scrambled static shares of 8 ranks are within 2 - 5 % of each other."""
    n = len(a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    hub = np.where(((lo + hi) & 1) == 0, lo, hi)
    order = np.argsort(hub, kind="stable")
    bounds = np.flatnonzero(np.diff(hub[order])) + 1
    groups = np.split(order, bounds)
    groups.sort(key=lambda g: ((int(hub[g[0]]) * 0x9E3779B1) & 0xFFFFFFFF, int(hub[g[0]])) if len(g) else (0, 0))
    out = [np.concatenate(groups[p::parts]) if groups[p::parts] else np.zeros(0, dtype=np.int64) for p in range(parts)]
    out = [c for c in out if len(c)]
    assert sum(len(c) for c in out) == n
    return out


def _shares_by_query(qa: np.ndarray, parts: int) -> List[np.ndarray]:
    """Indices of a sketch call's pair list dealt into `parts` shares (some may be empty): all pairs of one query genome in one
    share, the queries in id order handed to the share with the fewest pairs so far (ties: the first)."""
    order = np.argsort(qa, kind="stable")
    groups = np.split(order, np.flatnonzero(np.diff(qa[order])) + 1)
    shares, size = [[] for _ in range(parts)], [0] * parts
    for g in groups:
        p = size.index(min(size))
        shares[p].append(g); size[p] += len(g)
    return [np.concatenate(x) if x else np.zeros(0, dtype=np.int64) for x in shares]


class MultiEngine:
    """Engines on several devices behind the Engine calls the module functions use: genome store (replicated), anim_pairs / anib_pairs / sketch_pairs /
    anim_alignments_batch / anib_rows_batch (pairs pulled in chunks by the devices), tetra_counts / tetra_matrix (genomes counted in shards)."""

    def __init__(self, devices: Sequence[int], chunk_pairs: int = 0):
        if not devices:
            raise ValueError("MultiEngine needs at least one device")
        self.devices = list(devices)
        self.engines = [Engine(d) for d in self.devices]
        self.chunk_pairs = int(chunk_pairs)
        self.last_chunks_per_engine: List[int] = []

    # -- plumbing -------------------------------------------------------------------------------------------------------
    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _all(self, fn):
        """fn(engine) on every engine, one thread each; returns the results in engine order, re-raises the first error."""
        out, err = [None] * len(self.engines), []

        def run(k):
            try:
                out[k] = fn(self.engines[k])
            except BaseException as e:  # noqa: BLE001 — re-raised below
                err.append(e)
        ts = [threading.Thread(target=run, args=(k,)) for k in range(len(self.engines))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if err:
            raise err[0]
        return out

    # -- genome store: replicated ---------------------------------------------------------------------------------------
    def add_genome(self, seq, rec_off) -> int:
        ids = [e.add_genome(seq, rec_off) for e in self.engines]
        assert len(set(ids)) == 1
        return ids[0]

    def add_fasta(self, path):
        res = [e.add_fasta(path) for e in self.engines]
        assert len({r[0] for r in res}) == 1
        return res[0]

    def add_fasta_batch(self, paths, threads: int = 0):
        paths = list(paths)
        res = self._all(lambda e: e.add_fasta_batch(paths, threads))
        assert all(r == res[0] for r in res)
        return res[0]

    def genome_count(self) -> int:
        return self.engines[0].genome_count()

    def genome_length(self, gid: int):
        return self.engines[0].genome_length(gid)

    # heatmap clustering reads caller matrices only: one device is enough
    def cluster_pdist(self, x, columns: bool = False):
        return self.engines[0].cluster_pdist(x, columns)

    def cluster_linkage(self, x, method: int = 0, columns: bool = False):
        return self.engines[0].cluster_linkage(x, method, columns)

    def cluster_linkage_batch(self, problems):
        return self.engines[0].cluster_linkage_batch(problems)

    # ... and so does the neighbour-joining tree
    def tree_nj(self, d):
        return self.engines[0].tree_nj(d)

    def tree_nj_set(self, tail_limit: int = 512):
        return self.engines[0].tree_nj_set(tail_limit)

    def tree_nj_last(self):
        return self.engines[0].tree_nj_last()

    # ... and so do the distribution calls
    def dist_load(self, x):
        return self.engines[0].dist_load(x)

    def dist_hist(self, edges):
        return self.engines[0].dist_hist(edges)

    def dist_kde(self, points, bandwidth: float):
        return self.engines[0].dist_kde(points, bandwidth)

    def dist_release(self):
        return self.engines[0].dist_release()

    def clear_genomes(self):
        self._all(lambda e: e.clear_genomes())

    def upload(self):
        self._all(lambda e: e.upload())

    def anim_set_workers(self, workers: int = 2):
        """Engine.anim_set_workers on every device (host worker threads / streams per device)."""
        for e in self.engines:
            e.anim_set_workers(workers)

    def anib_set_search(self, mode: str):
        """Engine.anib_set_search on every device (the name is checked before any engine is touched)."""
        _lib.anib_search_code(mode)
        for e in self.engines:
            e.anib_set_search(mode)

    @property
    def anib_search(self) -> str:
        return self.engines[0].anib_search

    def anim_counters(self, reset: bool = False) -> np.ndarray:
        """Engine.anim_counters summed over the devices."""
        return np.sum([e.anim_counters(reset) for e in self.engines], axis=0).astype(np.uint64)

    # -- the work queue ----------------------------------------------------------------------------------------------------
    def _pull(self, chunks: List[np.ndarray], run_chunk, out: np.ndarray):
        lock = threading.Lock()
        first = {id(e): i for i, e in enumerate(self.engines)}      # engine i starts on chunk i (the static shares: one each) ...
        nxt = [min(len(self.engines), len(chunks))]                 # ... and then pulls what is left
        taken = defaultdict(int)

        def worker(e):
            k = first[id(e)]
            while True:
                if k >= len(chunks):
                    return
                idx = chunks[k]
                out[idx] = run_chunk(e, idx)
                taken[id(e)] += 1
                with lock:
                    k = nxt[0]
                    nxt[0] += 1
        self._all(worker)
        self.last_chunks_per_engine = [taken[id(e)] for e in self.engines]

    def _target(self, n: int) -> int:
        if self.chunk_pairs > 0:
            return self.chunk_pairs
        # ~24 chunks per device so that the tail is short, but never launches so small that the GPU idles inside them
        return max(2048, n // (24 * len(self.engines)) + 1)

    def anim_pairs(self, ref_ids, qry_ids, filter_1to1: bool = True, maxmatch: bool = False) -> np.ndarray:
        r = np.ascontiguousarray(list(ref_ids), dtype=np.int32)
        q = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        if len(r) != len(q):
            raise ValueError("ref_ids and qry_ids must have the same length")
        out = np.zeros(len(r), dtype=Engine.ANIM_DTYPE)
        if len(r):
            # one scrambled share per device, ONE call each (_static_parts_by_hub says why); chunk_pairs > 0: a queue of chunks of
            # that size, pulled by the devices (jobs whose cost is concentrated in a few genomes; the tests)
            chunks = (_chunks_by_hub(r, q, self.chunk_pairs) if self.chunk_pairs > 0
                      else _static_parts_by_hub(r, q, max(1, min(len(self.engines), len(r) // 64))))
            self._pull(chunks, lambda e, idx: e.anim_pairs(r[idx], q[idx], filter_1to1=filter_1to1, maxmatch=maxmatch), out)
        return out

    def anib_pairs(self, qry_ids, sbj_ids, fragsize: int = 1020) -> np.ndarray:
        qa = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        sa = np.ascontiguousarray(list(sbj_ids), dtype=np.int32)
        if len(qa) != len(sa):
            raise ValueError("qry_ids and sbj_ids must have the same length")
        out = np.zeros(len(qa), dtype=Engine.ANIB_DTYPE)
        if len(qa):
            self._pull(self._anib_chunks(qa), lambda e, idx: e.anib_pairs(qa[idx], sa[idx], fragsize), out)
        return out

    def _anib_chunks(self, qa: np.ndarray) -> List[np.ndarray]:
        """The pair list of a fragment-mode call cut for the devices: the fragmented (query) genome is the expensive side to set
        up — its pairs stay together (the genome is the hub of its chunk)."""
        order = np.argsort(qa, kind="stable")
        bounds = np.flatnonzero(np.diff(qa[order])) + 1
        groups, chunks, cur, size = np.split(order, bounds), [], [], 0
        target = max(64, len(qa) // (24 * len(self.engines)) + 1) if self.chunk_pairs <= 0 else self.chunk_pairs
        for g in groups:
            cur.append(g); size += len(g)
            if size >= target:
                chunks.append(np.concatenate(cur)); cur, size = [], 0
        if cur:
            chunks.append(np.concatenate(cur))
        return chunks

    # -- sketch mode ---------------------------------------------------------------------------------------------------------
    def sketch_pairs(self, qry_ids, ref_ids, frag_len: int = 3000, scale: int = 16, min_fraction: float = 0.2, kmer: int = 16,
                     mapping: str = "anywhere") -> np.ndarray:
        """Engine.sketch_pairs over all devices (mapping="window" included: the same deal).  The pairs are dealt by QUERY genome into one share per device — the pairs kernel
        streams a query's occurrence list once per up to four references, so a query's references belong together — ONE call per
        device; the records come back in the caller's order."""
        from . import _lib
        mapping = _lib.sketch_mapping(mapping)
        qa = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        ra = np.ascontiguousarray(list(ref_ids), dtype=np.int32)
        if len(qa) != len(ra):
            raise ValueError("qry_ids and ref_ids must have the same length")
        out = np.zeros(len(qa), dtype=Engine.SKETCH_DTYPE)
        if len(qa) == 0:
            return out
        shares = _shares_by_query(qa, len(self.engines))

        extra = () if mapping == "anywhere" else (mapping,)      # (the default call stays the call it was)

        def run(e):
            idx = shares[self.engines.index(e)]
            return e.sketch_pairs(qa[idx], ra[idx], frag_len, scale, min_fraction, kmer, *extra) if len(idx) else None
        for idx, res in zip(shares, self._all(run)):
            if res is not None:
                out[idx] = res
        return out

    # -- screen ----------------------------------------------------------------------------------------------------------------
    def screen_matrix(self, ids, kmer: int = 16, scale: int = 256, part: int = 0, n_parts: int = 1):
        """Engine.screen_matrix over all devices: the genome store is replicated, so the work is cut by slice bin, not by genome:
        device d of D takes part D * part + d of D * n_parts — together exactly the bins of the caller's part — and the host adds the
        integer results: equal to one engine's, whatever the number of devices."""
        ids = np.ascontiguousarray(list(ids), dtype=np.int32)
        d = len(self.engines)
        if d * int(n_parts) > 4096:      # more parts than slice bins: the devices beyond have nothing to take
            return self.engines[0].screen_matrix(ids, kmer, scale, part, n_parts)
        res = self._all(lambda e: e.screen_matrix(ids, kmer, scale, int(part) * d + self.engines.index(e), int(n_parts) * d))
        sizes = np.sum([r[0] for r in res], axis=0, dtype=np.uint64).astype(np.uint32)
        shared = np.sum([r[1] for r in res], axis=0, dtype=np.uint64).astype(np.uint32)
        return sizes, shared

    def screen_candidates(self, ids, options, labels=None, path: str = "auto"):
        """Engine.screen_candidates over all devices.  Dense path: the summed screen_matrix above, loaded onto the first engine, selected
        there.  Index path: EVERY engine builds the whole index — the store is replicated, and so is the scan, the sort
        and the grouping — and only the count and the selection are divided: engine d of D takes the bands d, d + D, ..., and the parts
        are merged by a stable sort on the row (a row lies in one band, so in one part).  What dividing only the back half is worth has
        not been measured.  Equal to one engine's on either path."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if screen.resolve_path(path, len(ids)) == "index":
            return screen.index_candidates_on(self.engines, lambda fn: self._all(lambda e: fn(e, self.engines.index(e))), ids, options, labels)
        first = self.engines[0]

        def make_resident():
            sizes, shared = self.screen_matrix(ids, options.kmer, options.scale)
            first.screen_load(shared)
            return sizes
        return screen.candidates_on(first, make_resident, ids, options, labels)

    def screen_components_of(self, ids, options, labels=None, path: str = "auto"):
        """Engine.screen_components_of over all devices.  Dense path: the first engine does the work.  Index path: every
        engine builds the whole index as for screen_candidates, engine d of D hooks and accumulates the kept cells of the bands d, d + D,
        ... into a forest of its own, and screen.merge_components joins the D forests on the first engine.  Equal to one engine's."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if screen.resolve_path(path, len(ids)) == "index":
            return screen.index_components_on(self.engines, lambda fn: self._all(lambda e: fn(e, self.engines.index(e))), ids, options, labels)
        return self.engines[0].screen_components_of(ids, options, labels, path="dense")

    def screen_search_index(self, ids, kmer: int = 16, scale: int = 256, labels=None):
        """Engine.screen_search_index over all devices: the collection is dealt into D contiguous ranges of call
        indices and engine d indexes its range ONLY, so the index's memory and its build time divide (fewer ranges than devices when the
        collection is that small: the engines beyond hold no index).  Returns the sizes in the order given.  A call that fails on any
        engine, for whatever reason, leaves NO index on any of them."""
        from . import screen
        ids = [int(i) for i in ids]
        labels = screen.search_labels(ids, labels, "db")
        d = len(self.engines)
        bounds = [len(ids) * k // d for k in range(d + 1)]
        self._search_ranges = [(bounds[k], bounds[k + 1]) for k in range(d)]

        def part(e):
            lo, hi = self._search_ranges[self.engines.index(e)]
            return e.screen_search_index(ids[lo:hi], kmer, scale, labels[lo:hi])
        try:
            sizes = np.concatenate(self._all(part)) if ids else np.zeros(0, np.uint32)
        except Exception:      # one engine's refusal or failure leaves the engines with indexes of different calls: none is kept
            self.screen_search_index_release()
            raise
        self._search = {"n": len(ids), "kmer": int(kmer), "scale": int(scale), "sizes": sizes, "labels": labels}
        return sizes

    def screen_search(self, query_ids, options, query_labels=None):
        """Engine.screen_search over all devices: every engine counts ALL queries against its range of the collection and selects
        locally — need_db depends on a db genome's own size only — and screen.merge_search_parts puts the parts together per query row
        with the ranges' column offsets added.  Equal to one engine's."""
        from . import screen
        options = screen.check_options(options)
        query_ids = [int(i) for i in query_ids]
        query_labels = screen.search_labels(query_ids, query_labels, "query")
        info = getattr(self, "_search", None)
        if not info or not info["n"]:
            raise ValueError("no search index on these engines (call screen_search_index first)")
        holders = [(e, lo) for e, (lo, hi) in zip(self.engines, self._search_ranges) if hi > lo]
        parts = self._all(lambda e: screen.search_chunks(e, query_ids, options) if any(e is h for h, _ in holders) else None)
        parts = [p for p in parts if p is not None]
        a, b, shared = screen.merge_search_parts([(lo, *p[1:]) for (_, lo), p in zip(holders, parts)])
        return screen.SearchHits(query_labels, list(info["labels"]), options, parts[0][0], info["sizes"], a, b, shared)

    def screen_search_index_release(self):
        for e in self.engines:
            e.screen_search_index_release()
        self._search, self._search_ranges = None, []

    # the index on disk and the remove are a single Engine's: here the collection is dealt in ranges of columns, one index each
    def screen_search_index_save(self, path, lengths=None):
        raise ValueError("a search index dealt over several devices cannot be saved: build it on a single Engine")

    def screen_search_index_load(self, path):
        raise ValueError("a search index file is loaded on a single Engine, not dealt over several devices")

    def screen_search_index_remove(self, which):
        raise ValueError("a search index dealt over several devices cannot be shrunk: remove on a single Engine")

    # the profile is a single Engine's for the same reason: every engine holds a range of the columns, and the occupancy of a
    # (k-mer, cluster) cell is a count over ALL of a cluster's columns
    def screen_search_profile(self, label, core: float = 0.95, shell: float = 0.15, marker_min_size: int = 2, thresholds=None):
        raise ValueError("a search index dealt over several devices cannot be profiled: build it on a single Engine")

    def screen_search_profile_last(self):
        raise ValueError("a search index dealt over several devices cannot be profiled: there is no profile to report on; use a single Engine")

    def screen_search_profile_release(self):
        raise ValueError("a search index dealt over several devices cannot be profiled: there is no profile to release; use a single Engine")

    def screen_search_profile_set(self, lane_limit=None, wave_limit=None, batch_keys: int = 0):
        raise ValueError("a search index dealt over several devices cannot be profiled: set the tiers on a single Engine")

    def screen_components(self, a, b, shared=None, n: int = 0):
        """Engine.screen_components on the first engine (a list call has nothing to divide)."""
        return self.engines[0].screen_components(a, b, shared, n=n)

    def screen_components_release(self):
        for e in self.engines:
            e.screen_components_release()

    def screen_representatives(self, a, b, weight=None, n: int = 0, score=None):
        """Engine.screen_representatives on the first engine (a list call has nothing to divide)."""
        return self.engines[0].screen_representatives(a, b, weight, n=n, score=score)

    def screen_representatives_release(self):
        for e in self.engines:
            e.screen_representatives_release()

    def screen_linkage(self, a, b, dist, n: int = 0, score=None, method: str = "average", cutoff: float = 0.05, fill: float = 1.0):
        """Engine.screen_linkage on the first engine (a list call has nothing to divide; dealing components is out of scope)."""
        return self.engines[0].screen_linkage(a, b, dist, n=n, score=score, method=method, cutoff=cutoff, fill=fill)

    def screen_linkage_set(self, small_limit=None, work_bytes: int = 0):
        for e in self.engines:
            e.screen_linkage_set(small_limit, work_bytes)

    def screen_linkage_last(self) -> dict:
        return self.engines[0].screen_linkage_last()

    def screen_linkage_release(self):
        for e in self.engines:
            e.screen_linkage_release()

    # the evaluation runs on the FIRST engine, as the linkage does: one list call has nothing to divide, and a dealt or
    # collective variant is out of scope.  The genome store is replicated, so the first engine's screen_evaluate_of sees every genome.
    def screen_evaluate(self, a, b, weight=None, n: int = 0, label=None, score=None):
        """Engine.screen_evaluate on the first engine (a list call has nothing to divide)."""
        return self.engines[0].screen_evaluate(a, b, weight, n=n, label=label, score=score)

    def screen_index_evaluate(self, need, label, score):
        """Engine.screen_index_evaluate on the first engine, over ITS resident index (all bands)."""
        return self.engines[0].screen_index_evaluate(need, label, score)

    def screen_evaluate_of(self, ids, options, label, scores=None, labels=None, path: str = "auto"):
        """Engine.screen_evaluate_of on the first engine alone (its own screen, not a dealt one).  Equal to one engine's."""
        return self.engines[0].screen_evaluate_of(ids, options, label, scores=scores, labels=labels, path=path)

    def screen_evaluate_last(self) -> dict:
        return self.engines[0].screen_evaluate_last()

    def screen_evaluate_release(self):
        for e in self.engines:
            e.screen_evaluate_release()

    def screen_dereplicate(self, ids, options, scores=None, labels=None, path: str = "auto"):
        """Engine.screen_dereplicate over all devices.  The greedy rule needs every entry in one place — a round reads
        the whole list, and a node's fate may hang on an entry of any band — so only the CANDIDATES are dealt as today
        (screen_candidates: the dense path's summed matrix, the index path's dealt bands, merged), and ONE list call runs on the first
        engine.  On the index path the kept pairs are therefore read back once, unlike one engine's.  Equal to one engine's."""
        from . import screen
        options = screen.check_options(options)
        ids = [int(i) for i in ids]
        if scores is not None and len(screen.score_keys(scores)) != len(ids):      # (refused before any work)
            raise ValueError(f"{len(ids)} genomes need {len(ids)} scores")
        try:
            return self.screen_candidates(ids, options, labels, path=path).representatives(scores, engine=self.engines[0])
        finally:
            self.engines[0].screen_representatives_release()

    def screen_set_budget(self, max_keys: int = 0):
        for e in self.engines:
            e.screen_set_budget(max_keys)

    def screen_set_band(self, rows: int = 0):
        for e in self.engines:
            e.screen_set_band(rows)

    def screen_last(self) -> dict:
        """Engine.screen_last of every device: the counts summed, the milliseconds of the slowest device per stage."""
        per = [e.screen_last() for e in self.engines]
        return {k: (max if k.endswith("_ms") else sum)(p[k] for p in per) for k in per[0]}

    def anib_rows_batch(self, qry_ids, sbj_ids, fragsize: int = 1020):
        """Engine.anib_rows_batch over all devices: the pair list is cut exactly as for anib_pairs, the devices pull chunks, and
        the parts are put back together in the caller's pair order (merge_anib_row_parts).  Returns (results, offsets, rows).
        Single-process only: pyani_amd.parallel.DistributedEngine has no such call, and there is no collective run_anib."""
        qa = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        sa = np.ascontiguousarray(list(sbj_ids), dtype=np.int32)
        if len(qa) != len(sa):
            raise ValueError("qry_ids and sbj_ids must have the same length")
        n = len(qa)
        if n == 0 or len(self.engines) == 1:
            return self.engines[0].anib_rows_batch(qa, sa, fragsize)
        chunks = self._anib_chunks(qa)
        parts = [None] * len(chunks)
        lock = threading.Lock()
        nxt = [0]

        def worker(e):
            while True:
                with lock:
                    k = nxt[0]
                    nxt[0] += 1
                if k >= len(chunks):
                    return
                idx = chunks[k]
                parts[k] = e.anib_rows_batch(qa[idx], sa[idx], fragsize)
        self._all(worker)
        return merge_anib_row_parts(n, chunks, parts)

    # -- alignment records (run_anim(write_output=True): the .delta / .filter files) -----------------------------------------------
    def anim_alignments_batch(self, ref_ids, qry_ids, maxmatch: bool = False, with_indels: bool = False):
        """Engine.anim_alignments_batch over all devices: the pair list is cut by hub genome as for anim_pairs, the devices pull
        chunks, and the records (and indel lists) are put back together in the caller's pair order."""
        r = np.ascontiguousarray(list(ref_ids), dtype=np.int32)
        q = np.ascontiguousarray(list(qry_ids), dtype=np.int32)
        if len(r) != len(q):
            raise ValueError("ref_ids and qry_ids must have the same length")
        n = len(r)
        if n == 0 or len(self.engines) == 1:
            return self.engines[0].anim_alignments_batch(r, q, maxmatch=maxmatch, with_indels=with_indels)
        # traceback launches keep their walks' pieces on the host: smaller chunks
        chunks = _chunks_by_hub(r, q, max(16 if with_indels else 256, n // (8 * len(self.engines)) + 1))
        parts = [None] * len(chunks)
        lock = threading.Lock()
        nxt = [0]

        def worker(e):
            while True:
                with lock:
                    k = nxt[0]
                    nxt[0] += 1
                if k >= len(chunks):
                    return
                idx = chunks[k]
                parts[k] = e.anim_alignments_batch(r[idx], q[idx], maxmatch=maxmatch, with_indels=with_indels)
        self._all(worker)
        return merge_alignment_parts(n, chunks, parts, with_indels)

    # -- TETRA: genomes are independent -> counted in shards, the small N x N matrix on one device ----------------------------
    def _id_shards(self, ids) -> List[np.ndarray]:
        ids = np.ascontiguousarray(list(ids), dtype=np.int32)
        if len(ids) == 0:
            return [ids]
        lens = np.array([self.engines[0].genome_length(int(g))[0] for g in ids], dtype=np.int64)
        # contiguous blocks of about equal bases (results are concatenated in order)
        cuts = np.searchsorted(np.cumsum(lens), np.linspace(0, lens.sum(), len(self.engines) + 1)[1:-1], side="left")
        return [b for b in np.split(ids, cuts) if len(b)]

    def tetra_counts(self, ids):
        shards = self._id_shards(ids)
        # one thread per engine through _all: an engine error (PG_E_NOMEM, a bad id) is re-raised here, not lost in a thread
        res = self._all(lambda e: e.tetra_counts(shards[self.engines.index(e)]) if self.engines.index(e) < len(shards) else None)
        res = [x for x in res if x is not None]
        return tuple(np.concatenate([x[j] for x in res]) for j in range(3))

    def tetra_matrix(self, ids, want_corr: bool = True):
        c2, c3, c4 = self.tetra_counts(ids)
        z, present = self.engines[0].tetra_zscores_from_counts(c2, c3, c4)
        corr = self.engines[0].tetra_corr(z, present) if want_corr else None
        return z, present, corr

    # -- single-pair / reduction calls go to the first engine ---------------------------------------------------------------
    def anim_pair_alignments(self, ref_id: int, qry_id: int):
        return self.engines[0].anim_pair_alignments(ref_id, qry_id)

    def anib_pair_rows(self, qry_id: int, sbj_id: int, fragsize: int = 1020):
        return self.engines[0].anib_pair_rows(qry_id, sbj_id, fragsize)

    def anim_reduce(self, pairs, apply_filter: bool = False):
        return self.engines[0].anim_reduce(pairs, apply_filter)

    def anib_reduce(self, pairs):
        return self.engines[0].anib_reduce(pairs)


def merge_alignment_parts(n: int, chunks: List[np.ndarray], parts, with_indels: bool):
    """Put the per-chunk results of Engine.anim_alignments_batch — (offsets, records, indel offsets, indels) over the chunk's own
    pairs — back into ONE result over the caller's n pairs, in the caller's order."""
    counts = np.zeros(n, dtype=np.int64)
    for idx, (off, _, _, _) in zip(chunks, parts):
        counts[idx] = np.diff(np.asarray(off, dtype=np.int64))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    total = int(offsets[-1])
    rec_dtype = next((p[1].dtype for p in parts if len(p[1])), Engine.ALN_DTYPE)
    recs = np.zeros(total, dtype=rec_dtype)
    icounts = np.zeros(total, dtype=np.int64)
    for idx, (off, rc, ioff, _) in zip(chunks, parts):
        off = np.asarray(off, dtype=np.int64)
        for j, p in enumerate(idx):
            a, b = int(off[j]), int(off[j + 1])
            if b > a:
                dst = int(offsets[p])
                recs[dst:dst + b - a] = rc[a:b]
                if with_indels:
                    icounts[dst:dst + b - a] = np.diff(np.asarray(ioff[a:b + 1], dtype=np.int64))
    if not with_indels:
        return offsets, recs, None, None
    ioffsets = np.zeros(total + 1, dtype=np.uint64)
    ioffsets[1:] = np.cumsum(icounts)
    ind_dtype = next((p[3].dtype for p in parts if p[3] is not None and len(p[3])), np.int64)
    indels = np.zeros(int(ioffsets[-1]), dtype=ind_dtype)
    for idx, (off, _, ioff, ind) in zip(chunks, parts):
        off = np.asarray(off, dtype=np.int64)
        for j, p in enumerate(idx):
            a, b = int(off[j]), int(off[j + 1])
            if b > a:
                dst = int(offsets[p])
                lo, hi = int(ioff[a]), int(ioff[b])
                indels[int(ioffsets[dst]):int(ioffsets[dst]) + hi - lo] = ind[lo:hi]
    return offsets, recs, ioffsets, indels


def merge_anib_row_parts(n: int, chunks: List[np.ndarray], parts):
    """Put the per-chunk results of Engine.anib_rows_batch — (results, offsets, rows) over the chunk's own pairs — back into ONE
    result over the caller's n pairs, in the caller's order.  chunks[k][j] is the caller's index of pair j of part k."""
    results = np.zeros(n, dtype=Engine.ANIB_DTYPE)
    counts = np.zeros(n, dtype=np.int64)
    for idx, (res, off, _) in zip(chunks, parts):
        if len(idx):
            results[idx] = res
            counts[idx] = np.diff(np.asarray(off, dtype=np.int64))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    rows = np.zeros(int(offsets[-1]), dtype=Engine.ANIB_ROW_DTYPE)
    for idx, (_, off, part_rows) in zip(chunks, parts):
        off = np.asarray(off, dtype=np.int64)
        for j, p in enumerate(idx):
            a, b = int(off[j]), int(off[j + 1])
            if b > a:
                dst = int(offsets[p])
                rows[dst:dst + b - a] = part_rows[a:b]
    return results, offsets, rows


def engine_for(devices: Optional[Iterable[int]] = None, workers: Optional[int] = None):
    """The engine a caller should use: `devices` as given; else `workers` GPUs starting at 0 (pyani's --workers, capped at the
    GPUs present); else the process-wide single engine."""
    from .engine import default_engine
    if devices is None and workers:
        import ctypes
        n = ctypes.c_int(0)
        try:
            hip = ctypes.CDLL("libamdhip64.so")
            if hip.hipGetDeviceCount(ctypes.byref(n)) != 0:
                n.value = 0
        except OSError:
            n.value = 0
        devices = list(range(max(1, min(int(workers), n.value or 1))))
    if devices is None:
        return default_engine()
    devices = list(devices)
    return MultiEngine(devices) if len(devices) > 1 or devices != [0] else default_engine()
