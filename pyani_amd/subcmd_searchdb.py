"""The screen's search index as a database one maintains: build it from a directory of FASTA files and SAVE it, then
update the file — genomes removed by label, genomes of another directory added — without reading the collection again.  This is
`skani sketch` / `sourmash index` for run_screen_search(index=) and run_screen_gather(index=): "build the database" apart from
"query it".  A genome is named by its file's stem, as everywhere; the file carries the stems, the genome lengths and the genomes' sizes
with the index's arrays, so a query run reads no FASTA file of the collection.

A single Engine only.  Both drivers release the search index when they return, and clear a genome store they own (one that was empty
when they began), on errors too.  OUT OF SCOPE: a MultiEngine (its collection is dealt in ranges of columns, one index each), a
compressed file, partial loads.
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import files, screen as screen_mod
from .engine import Engine, default_engine
from .subcmd_search import _stems, load_db


class IndexRun(NamedTuple):
    path: Path                      # the file written
    labels: List[str]               # the stems, in column order
    lengths: Dict[str, int]         # stem -> genome length
    sizes: np.ndarray               # uint32[n]: the genomes' sampled k-mers
    shape: tuple                    # (n, kmer, scale, D, E, n_slices, keys)
    file_bytes: int
    removed: List[str]              # run_screen_index_update: the stems taken out
    added: List[str]                # ... and the stems that joined


def _check_engine(engine) -> None:
    if engine is not None and not isinstance(engine, Engine):
        raise ValueError("a search index is built, saved and updated on a single Engine")


def _check_batch(db_batch) -> Optional[int]:
    if db_batch is None:
        return None
    if isinstance(db_batch, bool) or not isinstance(db_batch, (int, np.integer)) or int(db_batch) < 1:
        raise ValueError(f"db_batch must be an integer >= 1, not {db_batch!r}")
    return int(db_batch)


def _finish(eng, path, lengths: Dict[str, int], removed, added) -> IndexRun:
    info = eng._search
    if not info:
        raise ValueError("no genome is left: a search index of no genome is not saved")
    labels = list(info["labels"])
    shape = eng.screen_search_index_shape()
    size = eng.screen_search_index_save(path, lengths=[lengths[x] for x in labels])
    return IndexRun(Path(path), labels, {x: lengths[x] for x in labels}, np.array(info["sizes"], dtype=np.uint32), shape, size, list(removed), list(added))


def run_screen_index_build(db_dir, index_path, kmer: int = screen_mod.DEFAULT_KMER, scale: int = screen_mod.DEFAULT_SCALE,
                           db_batch: Optional[int] = None, engine: Optional[Engine] = None) -> IndexRun:
    """The search index of every FASTA file of `db_dir`, built as run_screen_search builds it (db_batch: that many files at a time
    through a store cleared after each batch) and saved to `index_path` with the stems and the genome lengths."""
    _check_engine(engine)
    db_batch = _check_batch(db_batch)
    kmer, scale = screen_mod.check_params(kmer, scale)
    eng = engine or default_engine()
    if db_batch is not None and eng.genome_count() != 0:
        raise ValueError("db_batch clears the genome store after every batch: it needs an engine whose store is empty")
    options = screen_mod.ScreenOptions(1.0, kmer, scale, screen_mod.DEFAULT_MIN_SHARED)      # (load_db reads kmer and scale only)
    db_paths = files.get_fasta_paths(Path(db_dir))
    db_stems = _stems(db_paths, "db")
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    try:
        load_db(eng, db_paths, db_stems, options, db_batch, lengths)
        return _finish(eng, index_path, lengths, [], db_stems)
    finally:
        eng.screen_search_index_release()
        if scratch_store:
            eng.clear_genomes()


def run_screen_index_update(index_path, add_dir=None, remove=None, out_path=None, db_batch: Optional[int] = None,
                            engine: Optional[Engine] = None) -> IndexRun:
    """The saved index `index_path` loaded, the genomes whose stems `remove` lists taken out (Engine.screen_search_index_remove), the
    FASTA files of `add_dir` added behind the rest (Engine.screen_search_index_add; db_batch files at a time) and the result saved to
    `out_path` (default: over `index_path`).  An unknown stem to remove, and a stem of `add_dir` that the index holds — after the
    removals: a genome is replaced by removing its stem and adding its new file in one call — are ValueErrors before a FASTA file is read."""
    _check_engine(engine)
    db_batch = _check_batch(db_batch)
    remove = [str(x) for x in (remove or [])]
    if len(set(remove)) != len(remove):
        raise ValueError("a stem to remove is given twice")
    add_paths = files.get_fasta_paths(Path(add_dir)) if add_dir is not None else []
    add_stems = _stems(add_paths, "added")
    f = screen_mod.read_search_index(index_path)
    held = set(f.labels)
    unknown = [x for x in remove if x not in held]
    if unknown:
        raise ValueError(f"the search index holds no genome {unknown[0]!r}")
    twice = [x for x in add_stems if x in held - set(remove)]
    if twice:
        raise ValueError(f"the search index already holds a genome {twice[0]!r}: remove it in the same call to replace it")
    eng = engine or default_engine()
    scratch_store = eng.genome_count() == 0
    if db_batch is not None and not scratch_store:
        raise ValueError("db_batch clears the genome store after every batch: it needs an engine whose store is empty")
    try:
        _, labels, stored = eng.screen_search_index_adopt(f, str(index_path))
        lengths = {x: int(v) for x, v in zip(labels, stored.tolist())}
        if remove:
            eng.screen_search_index_remove(remove)
        step = db_batch or max(len(add_paths), 1)
        for lo in range(0, len(add_paths), step):
            paths, stems = add_paths[lo:lo + step], add_stems[lo:lo + step]
            ids = []
            for p, (gid, total, _) in zip(paths, eng.add_fasta_batch(paths)):
                ids.append(gid)
                lengths[p.stem] = total
            if eng._search:
                eng.screen_search_index_add(ids, labels=stems)
            else:      # (every genome was removed: the index's kmer and scale start a new one)
                eng.screen_search_index(ids, f.shape[1], f.shape[2], labels=stems)
            if db_batch is not None:
                eng.clear_genomes()
        return _finish(eng, out_path if out_path is not None else index_path, lengths, remove, add_stems)
    finally:
        eng.screen_search_index_release()
        if scratch_store:
            eng.clear_genomes()
