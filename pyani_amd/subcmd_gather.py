"""The screen's gather over two directories of FASTA files: what each file of `query_dir` — a metagenome bin, a
contaminated assembly, a co-culture, loaded as ONE multi-record genome — is MADE OF, in genomes of the collection `db_dir`.  pyani has no
such step; this is `sourmash gather` put in front of pyani's ANIm: the collection is indexed ONCE (Engine.screen_search_index), each
query is counted against it with its matched k-mers kept on the device, and the greedy minimum set cover runs there: the db genome that
explains most of the query's still unexplained sampled k-mers is recorded with that count (unique) and its whole overlap (total), its
k-mers leave the query, and so on until no genome explains min_unique more.  A relative of a true member does not show up: the member
has already taken the k-mers they share.

There is NO default min_unique.  Two unrelated 5 Mb genomes share about 50 sampled 16-mers by chance at scale 256 (conserved genes and
low-complexity stretches, not random collisions), so a floor below that lists noise and the right floor depends on the genomes' size
and the scale; min_fraction adds a floor relative to the query's size.

Without exact= the collection's sequences are not needed after the index is built: a driver that owns the genome store clears it
before the queries are loaded.  With exact="anim" ONE anim_pairs call aligns (db genome as nucmer's reference, query) for the recorded
rows only, and each member's identity and coverage (of the member) are added to the rows' table.  The screen's own numbers stay an
ESTIMATE with its own files: `<outdir>/screen_output/gather_rows.tab` (one line per recorded genome) and `gather_summary.tab` (one per
query).  A single engine only.

abundance=True: a query of reads holds a member's k-mers as many times as it covers them, and sourmash gather's
abundance columns say how much of the sample each member accounts for.  The count then also keeps how many times the query holds each
matched k-mer, and every row gets the statistics of the multiplicities of the k-mers it claimed: average_abund, median_abund, std_abund,
f_unique_weighted, f_weighted_cumulative in the rows' table, weight, matched_weight, explained_weight, unexplained_weight in the
summary.  Abundance does not move a winner (as in sourmash): the rows, their order, unique and total are the unweighted gather's.

OUT OF SCOPE: a MultiEngine gather (the winner's k-mers live on one device: every round would need an exchange), FASTQ ingest (reads
come in as FASTA), a weighted CHOICE of winners (sourmash does not do it either), exact= from an index file, ANIb as exact=.

index=PATH: a saved search index takes the place of reading `db_dir` (None then), as for run_screen_search.
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import pandas as pd

from . import anim, files, screen as screen_mod
from .engine import Engine, default_engine
from .subcmd_screen import OUTDIR
from .subcmd_search import _stems, check_db_batch, check_index, load_db, load_index

EXACT = (None, "anim")


class GatherRun(NamedTuple):
    db_lengths: Dict[str, int]                  # stem -> genome length, file order
    query_lengths: Dict[str, int]
    result: screen_mod.GatherResult             # labels = the stems
    exact: Optional[Dict[Tuple[str, str], Tuple[int, int, float, int]]]      # exact="anim": (db stem, query stem) -> parse_delta tuple
    frame: pd.DataFrame                         # result.frame(), with the exact columns where they were asked for
    summary: pd.DataFrame                       # result.summary()
    written: List[Path]


def gather_tab_path(outdir, name: str) -> Path:
    return Path(outdir) / OUTDIR / f"gather_{name}.tab"


def run_screen_gather(db_dir, query_dir, outdir=None, min_unique: Optional[int] = None, kmer: int = screen_mod.DEFAULT_KMER,
                      scale: int = screen_mod.DEFAULT_SCALE, min_fraction: float = 0.0, max_ranks: int = screen_mod.GATHER_MAX_RANKS,
                      exact: Optional[str] = None, write_output: bool = False, engine: Optional[Engine] = None,
                      devices: Optional[List[int]] = None, workers: Optional[int] = None, db_batch: Optional[int] = None,
                      index=None, abundance: bool = False) -> GatherRun:
    """Every FASTA file of `query_dir` decomposed into the genomes of `db_dir`.  min_unique is required (there is no default threshold:
    about 50 sampled 16-mers are shared by chance between two unrelated 5 Mb genomes at scale 256); outdir is needed for write_output
    only.  devices / workers are refused: a gather runs on a single engine.  An engine holds ONE search index: one already resident on a
    caller's `engine` is replaced by the one of `db_dir`, and the engine holds none when this returns (released on errors too).
    db_batch: the collection goes through the store that many files at a time, each batch after the first ADDED to the resident index
    (run_screen_search's text); the result does not change.  index: the path of a saved search index in place of
    `db_dir` (None then): labels, lengths and every table column come from the file; without exact= and db_batch=.  abundance: the
    abundance columns are added to both tables (the module's text); with it off both are what they were without the option."""
    if min_unique is None:
        raise ValueError("run_screen_gather needs min_unique= (there is no default threshold)")
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")     # before any work is done
    if exact not in EXACT:
        raise ValueError(f"exact must be one of {EXACT}, not {exact!r}")
    if devices is not None or workers:
        raise ValueError("a gather runs on a single engine: devices= / workers= are not supported (the winner's k-mers live on one device)")
    options = screen_mod.check_gather_options(screen_mod.GatherOptions(kmer, scale, min_unique, min_fraction, max_ranks, abundance))
    index = check_index(index, db_dir, exact, db_batch, engine, None, None)
    db_batch = check_db_batch(db_batch, exact, engine, None, None)
    return _run(db_dir, query_dir, outdir, options, exact, write_output, engine or default_engine(), db_batch, index)


def _run(db_dir, query_dir, outdir, options, exact, write_output, eng, db_batch=None, index=None) -> GatherRun:
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
        result = eng.screen_gather(q_ids.tolist(), options, query_labels=q_stems)
        if exact == "anim":      # ONE call: the recorded rows only, the member as nucmer's reference
            results = {}
            if len(result.query):
                recs = eng.anim_pairs(db_ids[result.db], q_ids[result.query])
                for rec, a, b in zip(recs, result.query.tolist(), result.db.tolist()):
                    try:
                        results[(db_stems[b], q_stems[a])] = anim._tuple(rec)
                    except ZeroDivisionError:      # no alignment: the row has no exact value (NaN in the table)
                        pass
    finally:
        eng.screen_search_index_release()
        if scratch_store:
            eng.clear_genomes()
    frame = result.frame()
    if results is not None:
        nan4 = (0, 0, float("nan"), 0)
        got = [results.get((d, q), nan4) for q, d in zip(frame["query"], frame["db"])]
        frame["anim_identity"] = np.array([r[2] for r in got], dtype=np.float64)
        frame["anim_coverage_db"] = np.array([r[0] / db_len[d] if r is not nan4 and db_len[d] else np.nan for r, d in zip(got, frame["db"])], dtype=np.float64)
    summary = result.summary()
    written: List[Path] = []
    if write_output:
        (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
        frame.to_csv(gather_tab_path(outdir, "rows"), index=False, sep="\t")
        summary.to_csv(gather_tab_path(outdir, "summary"), index=False, sep="\t")
        written = [gather_tab_path(outdir, "rows"), gather_tab_path(outdir, "summary")]
    return GatherRun(db_len, q_len, result, results, frame, summary, written)
