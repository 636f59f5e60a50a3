"""`pyani fastani` without the fastANI binary: the driver of pyani/scripts/subcommands/subcmd_fastani.py:114-480 with its one
`fastANI -q ... -r ...` job per ordered pair replaced by ONE batched GPU call of the sketch mode (pyani_amd/fastani.py,
pg_sketch_pairs_k).  No CLI and no database — the result tuples, Comparison rows and matrices come back as plain data.

What is kept of the reference's behaviour:
  * inputs: the FASTA files of `indir` in sorted order; all N(N-1) ordered pairs with query != reference
    (`permutations(genomes, 2)`, subcmd_fastani.py:227);
  * parameters: fragLen, kmerSize (8 ... 16) and minFraction (fastani_parser.py:100-132);
  * output files, all under `<outdir>/fastani_output/`: one `<q>_vs_<r>.fastani` per ordered pair, the line fastANI prints (full
    input paths, query first, ANI in percent to 4 places, matches, fragments) or an EMPTY file where there is no result;
  * `recovery=True`: pairs whose file already exists are NOT computed — the file (fastANI's or ours) is parsed, an empty one is
    a recovered "no result" — the others go to the engine in one call;
  * rows: update_comparison_results' Comparison row per pair (subcmd_fastani.py:437-476; an empty file becomes the (0, 0, 0) row);
  * matrices: update_comparison_matrices' five frames (pyani_orm.py:618-666) made from those rows by anim.assemble_run_matrices.

The reference's driver only ever sees the files (ANI as a percentage with 4 decimals).  Here a run with write_output=True does the
same — its results are its own files read back, so that a later recovery run over them gives equal results — while a run that
writes nothing returns the engine's estimates at full precision.

These are the sketch mode's OWN matrices: an estimate, never merged into an ANIm or ANIb result.  Single-process: one
engine, or several GPUs of this node through pyani_amd.multi.MultiEngine (devices / workers).
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import pandas as pd

from . import anim, fastani, files
from .engine import Engine, default_engine

ALIGNDIR = "fastani_output"     # pyani_config.ALIGNDIR["fastANI"]


class FastaniRun(NamedTuple):
    lengths: Dict[str, int]                                                   # stem -> genome length
    results: Dict[Tuple[str, str], Optional[fastani.ComparisonResult]]       # (query stem, reference stem), the run's pair order
    rows: List[dict]                                                          # fastani.comparison_row per pair, same order
    matrices: Dict[str, pd.DataFrame]                                         # the five frames of update_comparison_matrices
    recovered: List[Path]                                                     # result files reused in recovery mode
    written: List[Path]                                                       # result files written by this run


def result_path(outdir: Path, qstem: str, rstem: str) -> Path:
    """fastani.py:215: `<query stem>_vs_<reference stem>.fastani`, strings appended (stems may contain dots)."""
    return Path(outdir) / ALIGNDIR / (f"{qstem}_vs_{rstem}" + ".fastani")


def run_fastani(indir, outdir=None, fragLen: int = 3000, kmerSize: int = 16, minFraction: float = 0.2, recovery: bool = False,
                write_output: bool = False, engine: Optional[Engine] = None, devices: Optional[List[int]] = None,
                workers: Optional[int] = None, mapping: str = "anywhere") -> FastaniRun:
    """The sketch mode over every FASTA file of `indir`.  outdir is needed for recovery / write_output only.
    devices / workers: run on several GPUs of this node (pyani_amd/multi.py); ignored when `engine` is given.
    mapping: "anywhere" (default) or "window" (fastani.calculate_fastani_pairs).  Files, rows and matrices keep their shape.  A
    recovery run trusts the files it finds: as with kmerSize, the caller keeps ONE outdir per mapping."""
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")     # before any work is done
    if recovery and outdir is None:
        raise ValueError("recovery mode needs the output directory of the earlier run")
    kmerSize = fastani.check_kmer(kmerSize)
    from . import _lib
    mapping = _lib.sketch_mapping(mapping)
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        return _run_fastani(indir, outdir, fragLen, kmerSize, minFraction, recovery, write_output, engine or default_engine(), mapping)
    finally:
        if own is not None:
            own.close()


def _parsed(path: Path) -> Optional[fastani.ComparisonResult]:
    try:
        return fastani.parse_fastani_file(path)
    except fastani.PyaniFastANIException:      # an empty file: no result (subcmd_fastani.py:437-441)
        return None


def _run_fastani(indir, outdir, fragLen, kmerSize, minFraction, recovery, write_output, eng, mapping="anywhere") -> FastaniRun:
    paths = files.get_fasta_paths(Path(indir))
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError("two input files share a stem (pyani keys every result by Path.stem)")
    by_stem = dict(zip(stems, paths))
    order = [(q, r) for q in stems for r in stems if q != r]      # permutations(genomes, 2)
    todo = list(order)
    results: Dict[Tuple[str, str], Optional[fastani.ComparisonResult]] = {}
    recovered: List[Path] = []
    if recovery:
        for q, r in order:
            f = result_path(outdir, q, r)
            if f.is_file():
                results[(q, r)] = _parsed(f)
                recovered.append(f)
        todo = [k for k in order if k not in results]
    written: List[Path] = []
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    try:
        ids = {}
        for p, (gid, total, _) in zip(paths, eng.add_fasta_batch(paths)):
            ids[p.stem], lengths[p.stem] = gid, total
        if todo:
            recs = fastani.calculate_fastani_pairs(eng, [ids[q] for q, _ in todo], [ids[r] for _, r in todo], fragLen, kmerSize, minFraction, mapping=mapping)
            if write_output:
                (Path(outdir) / ALIGNDIR).mkdir(parents=True, exist_ok=True)
            for (q, r), x in zip(todo, recs):
                # field order: the reference's positional quirk, as fastani.comparison_results (the QUERY file lands in `.reference`)
                res = None if int(x["status"]) else fastani.ComparisonResult(by_stem[q], by_stem[r], float(x["ani"]), int(x["matches"]), int(x["fragments"]))
                if write_output:
                    f = fastani.write_fastani_file(result_path(outdir, q, r), by_stem[q], by_stem[r], res)
                    written.append(f)
                    res = _parsed(f)      # what the reference's driver sees, and what a recovery run over this file will see
                results[(q, r)] = res
    finally:
        if scratch_store:
            eng.clear_genomes()
    results = {k: results[k] for k in order}      # the run's pair order, whatever was recovered
    rows = [fastani.comparison_row(results[(q, r)], by_stem[q], by_stem[r], fragLen, lengths[q], kmerSize, minFraction) for q, r in order]
    cells = {k: (row["aln_length"], row["aln_length"], row["identity"], row["sim_errs"]) for k, row in zip(order, rows)}
    return FastaniRun(lengths, results, rows, anim.assemble_run_matrices(cells, lengths), recovered, written)
