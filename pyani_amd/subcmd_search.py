"""The screen's search over two directories of FASTA files: which genomes of a collection (`db_dir`) each new genome
(`query_dir`) is related to, and how closely.  pyani has no such step; this is `skani search` / `sourmash search` put in front of
pyani's ANIm: the collection is indexed ONCE (Engine.screen_search_index: every distinct sampled k-mer with its holders, resident on
the device), the queries are counted against it and the kept (query, db genome) cells come back — never a db x db cell.

Without exact= the collection's sequences are not needed after the index is built: a driver that owns the genome store clears it
before the queries are loaded (the index survives pg_clear_genomes).  With exact="anim" ONE anim_pairs call aligns every kept pair in
both directions — built from the SearchHits arrays, the query as nucmer's reference for the forward direction, as in run_anim — and
the identity and coverage of both directions are added to the hits' table.  The screen's own numbers stay an ESTIMATE with its own
files: `<outdir>/screen_output/search_hits.tab` (every kept cell) and `search_best.tab` (per query its `top` hits, default 1).
OUT OF SCOPE: ANIb as exact=, exact= from an index file, recovery, collective runs.  Single-process: one engine, or several GPUs of this node
(devices / workers: the collection is dealt over them, MultiEngine.screen_search_index).

db_batch=N: the collection is loaded N files at a time — the first batch is indexed, every later one ADDED to the
resident index (Engine.screen_search_index_add), the store cleared after each — so a collection larger than the genome arena can be
searched.  Only for a run that owns the store, on a single Engine, without exact= (the sequences are gone).  The result is the same.

index=PATH: a search index saved by subcmd_searchdb.run_screen_index_build (or Engine.screen_search_index_save) takes
the place of reading `db_dir`, which must then be None: the db labels, lengths and every table column come from the file, and not a
FASTA file of the collection is read.  On a single Engine, without exact= (the file holds no sequence) and without db_batch=.
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import pandas as pd

from . import anim, files, screen as screen_mod
from .engine import Engine, default_engine
from .subcmd_screen import OUTDIR

EXACT = (None, "anim")


class SearchRun(NamedTuple):
    db_lengths: Dict[str, int]                  # stem -> genome length, file order
    query_lengths: Dict[str, int]
    hits: screen_mod.SearchHits                 # labels = the stems
    best: screen_mod.SearchHits                 # hits.best(top or 1)
    exact: Optional[Dict[Tuple[str, str], Tuple[int, int, float, int]]]      # exact="anim": (nucmer's reference stem, query stem) -> parse_delta tuple, both directions
    frame: pd.DataFrame                         # hits.frame(), with the exact columns where they were asked for
    written: List[Path]


def search_tab_path(outdir, name: str) -> Path:
    return Path(outdir) / OUTDIR / f"search_{name}.tab"


def _stems(paths, what: str) -> List[str]:
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError(f"two {what} files share a stem (pyani keys every result by Path.stem)")
    return stems


def check_db_batch(db_batch, exact, engine, devices, workers) -> Optional[int]:
    """The db_batch= of run_screen_search and run_screen_gather, checked before a file is read or an engine is made: None, or an integer
    >= 1 on a single Engine whose store is empty, without exact=."""
    if db_batch is None:
        return None
    if isinstance(db_batch, bool) or not isinstance(db_batch, (int, np.integer)) or int(db_batch) < 1:
        raise ValueError(f"db_batch must be an integer >= 1, not {db_batch!r}")
    if exact is not None:
        raise ValueError("db_batch clears the store after every batch: exact= needs the collection's sequences and cannot go with it")
    if devices is not None or workers or (engine is not None and not isinstance(engine, Engine)):
        raise ValueError("db_batch runs on a single Engine: a collection dealt over several devices cannot be added to")
    if engine is not None and engine.genome_count() != 0:
        raise ValueError("db_batch clears the genome store after every batch: it needs an engine whose store is empty")
    return int(db_batch)


def check_index(index, db_dir, exact, db_batch, engine, devices, workers) -> Optional[str]:
    """The index= of run_screen_search and run_screen_gather, checked before a file is read or an engine is made: None (then db_dir is
    needed), or the path of a saved search index in place of db_dir, on a single Engine, without exact= and db_batch=."""
    if index is None:
        if db_dir is None:
            raise ValueError("a collection is needed: db_dir=, or index= with a saved search index")
        return None
    if db_dir is not None:
        raise ValueError("index= takes the place of db_dir: give one of them (db_dir=None with index=)")
    if exact is not None:
        raise ValueError("index= holds no sequence of the collection: exact= needs db_dir")
    if db_batch is not None:
        raise ValueError("index= reads no file of a collection: db_batch= goes with db_dir")
    if devices is not None or workers or (engine is not None and not isinstance(engine, Engine)):
        raise ValueError("index= runs on a single Engine: a saved search index is not dealt over several devices")
    return str(index)


def load_index(eng, index, options, db_len):
    """The saved search index `index` made resident on `eng` in place of load_db: (positions, db labels); db_len is filled from the file.
    A file of another kmer or scale than the options' is a ValueError after its header is read and before anything is uploaded."""
    f = screen_mod.read_search_index(index)
    if (f.shape[1], f.shape[2]) != (options.kmer, options.scale):
        raise ValueError(f"{index}: the search index was built with kmer {f.shape[1]} and scale {f.shape[2]}, not {options.kmer} and {options.scale}")
    _, labels, lengths = eng.screen_search_index_adopt(f, index)
    for stem, length in zip(labels, lengths.tolist()):
        db_len[stem] = int(length)
    return np.arange(len(labels), dtype=np.int64), labels


def load_db(eng, db_paths, db_stems, options, db_batch, db_len) -> np.ndarray:
    """The collection's files loaded and the search index built: in one piece (returns the genomes' ids), or db_batch files at a time
    through a store cleared after every batch (the ids are gone with the sequences: positions are returned)."""
    if db_batch is None:
        db_ids = np.zeros(len(db_paths), dtype=np.int64)
        for k, (p, (gid, total, _)) in enumerate(zip(db_paths, eng.add_fasta_batch(db_paths))):
            db_ids[k], db_len[p.stem] = gid, total
        eng.screen_search_index(db_ids.tolist(), options.kmer, options.scale, labels=db_stems)
        return db_ids
    if eng.genome_count() != 0:      # (the default engine is known only now)
        raise ValueError("db_batch clears the genome store after every batch: it needs an engine whose store is empty")
    if not db_paths:
        eng.screen_search_index([], options.kmer, options.scale, labels=[])
    for lo in range(0, len(db_paths), db_batch):
        paths, stems = db_paths[lo:lo + db_batch], db_stems[lo:lo + db_batch]
        ids = []
        for p, (gid, total, _) in zip(paths, eng.add_fasta_batch(paths)):
            ids.append(gid)
            db_len[p.stem] = total
        if lo == 0:
            eng.screen_search_index(ids, options.kmer, options.scale, labels=stems)
        else:
            eng.screen_search_index_add(ids, labels=stems)
        eng.clear_genomes()
    return np.arange(len(db_paths), dtype=np.int64)


def run_screen_search(db_dir, query_dir, outdir=None, min_identity: Optional[float] = None, kmer: int = screen_mod.DEFAULT_KMER,
                      scale: int = screen_mod.DEFAULT_SCALE, min_shared: int = screen_mod.DEFAULT_MIN_SHARED, top: Optional[int] = None,
                      exact: Optional[str] = None, write_output: bool = False, engine: Optional[Engine] = None,
                      devices: Optional[List[int]] = None, workers: Optional[int] = None, db_batch: Optional[int] = None,
                      index=None) -> SearchRun:
    """Every FASTA file of `query_dir` placed against the collection of `db_dir`.  min_identity is required (there is no default
    threshold); outdir is needed for write_output only; devices / workers: several GPUs of this node, ignored when `engine` is given.
    An engine holds ONE search index: a search index already resident on a caller's `engine` is replaced by the one of `db_dir`, and
    the engine holds none when this returns (released on errors too).  db_batch: the collection goes through the store that many files
    at a time (the module's text); the result does not change.  index: the path of a saved search index in place of `db_dir` (None
    then; the module's text)."""
    if min_identity is None:
        raise ValueError("run_screen_search needs min_identity= (there is no default threshold)")
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")     # before any work is done
    if exact not in EXACT:
        raise ValueError(f"exact must be one of {EXACT}, not {exact!r}")
    if top is not None and (isinstance(top, bool) or int(top) != top or int(top) < 1):
        raise ValueError(f"top must be an integer >= 1, not {top!r}")
    options = screen_mod.check_options(screen_mod.ScreenOptions(min_identity, kmer, scale, min_shared))
    index = check_index(index, db_dir, exact, db_batch, engine, devices, workers)
    db_batch = check_db_batch(db_batch, exact, engine, devices, workers)
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        return _run(db_dir, query_dir, outdir, options, int(top or 1), exact, write_output, engine or default_engine(), db_batch, index)
    finally:
        if own is not None:
            own.close()


def _coverage(aln: int, length: int) -> float:
    return aln / length if length else float("nan")


def _run(db_dir, query_dir, outdir, options, top, exact, write_output, eng, db_batch=None, index=None) -> SearchRun:
    db_paths, q_paths = files.get_fasta_paths(Path(db_dir)) if index is None else [], files.get_fasta_paths(Path(query_dir))
    db_stems, q_stems = _stems(db_paths, "db"), _stems(q_paths, "query")
    scratch_store = eng.genome_count() == 0
    db_len: Dict[str, int] = {}
    q_len: Dict[str, int] = {}
    results = None
    try:
        if index is None:
            db_ids = load_db(eng, db_paths, db_stems, options, db_batch, db_len)
        else:
            db_ids, db_stems = load_index(eng, index, options, db_len)
        if exact is None and scratch_store:      # the index names the collection by position only: its sequences make room for the queries
            eng.clear_genomes()
        q_ids = np.zeros(len(q_paths), dtype=np.int64)
        for k, (p, (gid, total, _)) in enumerate(zip(q_paths, eng.add_fasta_batch(q_paths))):
            q_ids[k], q_len[p.stem] = gid, total
        hits = eng.screen_search(q_ids.tolist(), options, query_labels=q_stems)
        if exact == "anim" and len(hits.a):      # ONE call: the kept pairs with the query as nucmer's reference, then the other way round
            ref = np.concatenate([q_ids[hits.a], db_ids[hits.b]])
            qry = np.concatenate([db_ids[hits.b], q_ids[hits.a]])
            recs = eng.anim_pairs(ref, qry)
            m = len(hits.a)
            results = {}
            for k, (a, b) in enumerate(zip(hits.a.tolist(), hits.b.tolist())):
                for key, rec in (((q_stems[a], db_stems[b]), recs[k]), ((db_stems[b], q_stems[a]), recs[m + k])):
                    try:
                        results[key] = anim._tuple(rec)
                    except ZeroDivisionError:      # no alignment: the pair has no exact value (NaN in the table)
                        pass
        elif exact == "anim":
            results = {}
    finally:
        eng.screen_search_index_release()
        if scratch_store:
            eng.clear_genomes()
    frame = hits.frame()
    if results is not None:
        nan4 = (0, 0, float("nan"), 0)
        fwd = [results.get((q, d), nan4) for q, d in zip(frame["query"], frame["db"])]
        rev = [results.get((d, q), nan4) for q, d in zip(frame["query"], frame["db"])]
        frame["anim_identity_query"] = np.array([r[2] for r in fwd], dtype=np.float64)
        frame["anim_coverage_query"] = np.array([_coverage(r[0], q_len[q]) if r is not nan4 else np.nan for r, q in zip(fwd, frame["query"])], dtype=np.float64)
        frame["anim_identity_db"] = np.array([r[2] for r in rev], dtype=np.float64)
        frame["anim_coverage_db"] = np.array([_coverage(r[0], db_len[d]) if r is not nan4 else np.nan for r, d in zip(rev, frame["db"])], dtype=np.float64)
    best = hits.best(top)
    written: List[Path] = []
    if write_output:
        (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
        frame.to_csv(search_tab_path(outdir, "hits"), index=False, sep="\t")
        best.frame().to_csv(search_tab_path(outdir, "best"), index=False, sep="\t")
        written = [search_tab_path(outdir, "hits"), search_tab_path(outdir, "best")]
    return SearchRun(db_len, q_len, hits, best, results, frame, written)
