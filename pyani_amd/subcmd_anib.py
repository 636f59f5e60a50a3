"""`average_nucleotide_identity.py -m ANIb` without BLAST+: the driver of the legacy script's unified_anib
(pyani/scripts/average_nucleotide_identity.py:694-765) with its makeblastdb / blastn jobs replaced by batched GPU calls.  No CLI —
the tuples and matrices come back as plain data.

What is kept of the reference's behaviour:
  * inputs: the FASTA files of `indir` in sorted order (pyani_files.get_fasta_paths); all N(N-1) ordered pairs are compared
    (generate_blastn_commands, anib.py:383-420: every fragment file against every other genome);
  * output files, all under `<outdir>/blastn_output/` (pyani_config.ALIGNDIR["ANIb"]): the fragment files
    `<stem>-fragments<suffix>` (fragment_fasta_files, anib.py:164-203) and one table `<q>_vs_<s>.blast_tab` per ordered pair in the
    15 columns pyani asks blastn for (anib.py:451-471);
  * `recovery=True` is the script's `--skip_blastn`: pairs whose table already exists are NOT searched — the file (BLAST+'s or
    ours) is parsed and reduced instead (process_blast -> parse_blast_tab, anib.py:496-667) — the others are run;
  * results: parse_blast_tab's tuple per ordered pair and process_blast's five matrices (anib.process_blast_results);
  * errors: a pair the engine could not process raises RuntimeError, as calculate_anib_pairs does.

  * `search` picks the engine's search mode for the run (Engine.anib_set_search; the engine's own setting comes back afterwards).  A
    run that writes its tables also writes `<outdir>/anib_run.json` naming the mode, and recovery refuses a directory whose record
    names the other one: tables of two modes are not mixed silently.  A directory without a record (BLAST+'s own tables, or an
    earlier version's) counts as "seeds".

  * `screen` (pyani_amd.screen.ScreenOptions, or a bare identity threshold) searches only the pairs the k-mer screen keeps
    (Engine.screen_candidates).  A dropped pair has no tuple and no table, and its cells are NaN in all five matrices —
    not the 1.0 / 0 process_blast starts from, which would read as a perfect match.  The options are part of the run record, and
    recovery refuses a directory recorded with other options (or with none), as it does for another search mode.

Single-process: one engine, or several GPUs of this node through pyani_amd.multi.MultiEngine (devices / workers).  There is no
collective (one process per GPU) run_anib: pyani_amd.parallel.DistributedEngine has no rows call.
"""
import json
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import pandas as pd

import numpy as np

from . import _lib, anib, anim, files, screen as screen_mod
from .engine import Engine, default_engine

ALIGNDIR = "blastn_output"     # pyani_config.ALIGNDIR["ANIb"]


class AnibRun(NamedTuple):
    lengths: Dict[str, int]                                     # stem -> genome length
    fraglengths: Optional[Dict[str, Dict[str, int]]]            # fragment_fasta_files' dict; None unless fragment files were written
    results: Dict[Tuple[str, str], Tuple[int, int, float]]      # (query stem, subject stem) -> parse_blast_tab tuple
    matrices: Dict[str, pd.DataFrame]                           # process_blast_results
    recovered: List[Path]                                       # tables reused in recovery mode
    written: List[Path]                                         # tables written by this run
    screened: Optional[screen_mod.ScreenedPairs] = None         # the pairs the screen kept (screen=...), None for an unscreened run


WRITE_CHUNK = 256      # ordered pairs per anib_rows_batch call of write_output (its rows are held on the host)


def fragment_path(outdir: Path, fasta: Path) -> Path:
    """anib.py:190: the suffix is appended to the stem as a string (stems may contain dots)."""
    fasta = Path(fasta)
    return Path(outdir) / ALIGNDIR / f"{fasta.stem}-fragments{fasta.suffix}"


def table_path(outdir: Path, qstem: str, sstem: str) -> Path:
    """anib.py:464-466: `<query stem>_vs_<subject stem>.blast_tab`, strings appended (stems may contain dots)."""
    return Path(outdir) / ALIGNDIR / (f"{qstem}_vs_{sstem}" + ".blast_tab")


RUN_RECORD = "anib_run.json"   # <outdir>/anib_run.json: {"search": ..., "screen": ...} of the run that wrote the tables


def recorded_search(outdir) -> str:
    """The search mode the tables under `outdir` were written with; "seeds" when the directory holds no run record."""
    f = Path(outdir) / RUN_RECORD
    if not f.is_file():
        return "seeds"
    with open(f) as fh:
        return str(json.load(fh).get("search", "seeds"))


def recorded_screen(outdir) -> Optional[dict]:
    """The screen options the tables under `outdir` were written with, as the record holds them; None for an unscreened run or a
    directory without a record."""
    f = Path(outdir) / RUN_RECORD
    if not f.is_file():
        return None
    with open(f) as fh:
        return json.load(fh).get("screen")


def run_anib(indir, outdir=None, fragsize: int = anib.FRAGSIZE, recovery: bool = False, write_output: bool = False,
             engine: Optional[Engine] = None, devices: Optional[List[int]] = None, workers: Optional[int] = None,
             search: str = "seeds", screen=None) -> AnibRun:
    """ANIb over every FASTA file of `indir`.  outdir is needed for recovery / write_output only.
    devices / workers: run on several GPUs of this node (pyani_amd/multi.py); ignored when `engine` is given.
    search: "seeds" (default) or "all_diagonals" (Engine.anib_set_search) for this run.
    screen: None (default: all N(N-1) pairs), or a ScreenOptions / a bare identity threshold: after the genomes are loaded and recovery
    has taken the pairs whose tables exist, the screen runs over ALL genomes of the run and the pairs still to do are cut down to the
    ones it keeps, in their order.  There is no default threshold — DESIGN.md §16: on C4 0.80 kept every covered pair and dropped
    97.8 % of all pairs, 0.85 already lost relatives.  min_identity <= 0 keeps every pair (the run equals the unscreened one)."""
    _lib.anib_search_code(search)     # before any work is done
    if screen is not None:
        screen = screen_mod.check_options(screen)
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")
    if recovery and outdir is None:
        raise ValueError("recovery mode needs the output directory of the earlier run")
    if recovery and recorded_search(outdir) != search:
        raise ValueError(f"recovery: the tables under {outdir} were written with search={recorded_search(outdir)!r}, this run asks for "
                         f"{search!r}; the two modes' tables are not mixed")
    screen_record = None if screen is None else dict(screen._asdict())
    if recovery and recorded_screen(outdir) != screen_record:
        raise ValueError(f"recovery: the tables under {outdir} were written with screen={recorded_screen(outdir)!r}, this run asks for "
                         f"{screen_record!r}; a directory holds the tables of one selection")
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        eng = engine or default_engine()
        with anib.search_mode(eng, search):
            run = _run_anib(indir, outdir, fragsize, recovery, write_output, eng, screen)
        if write_output:
            with open(Path(outdir) / RUN_RECORD, "w") as fh:
                json.dump({"search": search, "fragsize": int(fragsize), **({} if screen is None else {"screen": screen_record})}, fh)
                fh.write("\n")
        return run
    finally:
        if own is not None:
            own.close()


def _tuple(q: str, s: str, rec) -> Tuple[int, int, float]:
    if int(rec["status"]) != 0:
        raise RuntimeError(f"GPU ANIb comparison {q} vs {s} failed with status {int(rec['status'])}")
    return int(rec["aln_length"]), int(rec["sim_errors"]), float(rec["pid"])


def _run_anib(indir, outdir, fragsize, recovery, write_output, eng, screen=None) -> AnibRun:
    paths = files.get_fasta_paths(Path(indir))
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError("two input files share a stem (pyani keys every result by Path.stem)")
    by_stem = dict(zip(stems, paths))
    todo = [(q, s) for q in stems for s in stems if q != s]
    results: Dict[Tuple[str, str], Tuple[int, int, float]] = {}
    recovered: List[Path] = []
    if recovery:
        old = [(q, s, table_path(outdir, q, s)) for q, s in todo]
        old = [(q, s, f) for q, s, f in old if f.is_file()]
        if old:
            aln, err, pid = eng.anib_reduce([anib.read_blast_tab(f) for _, _, f in old])
            for k, (q, s, f) in enumerate(old):
                results[(q, s)] = (int(aln[k]), int(err[k]), float(pid[k]))
                recovered.append(f)
        done = {(q, s) for q, s, _ in old}
        todo = [k for k in todo if k not in done]
    written: List[Path] = []
    fraglengths = None
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    try:
        ids = {}
        for p, (gid, total, _) in zip(paths, eng.add_fasta_batch(paths)):
            ids[p.stem], lengths[p.stem] = gid, total
        screened = None
        if screen is not None:
            screened = eng.screen_candidates([ids[s] for s in stems], screen, labels=stems)
            kept = {(stems[a], stems[b]) for a, b in screened.pairs()}
            todo = [k for k in todo if k in kept]
            if write_output:
                from .subcmd_screen import write_pairs_tab
                write_pairs_tab(outdir, screened)
        if write_output:
            (Path(outdir) / ALIGNDIR).mkdir(parents=True, exist_ok=True)
            _, fraglengths = anib.fragment_fasta_files(paths, Path(outdir) / ALIGNDIR, fragsize)
        if todo and write_output:
            # the tables the blastn jobs would have left: batched calls, the tuples from the same call (no pair is searched twice)
            subject = {}      # record ids and lengths of a subject genome: read once per genome
            for c0 in range(0, len(todo), WRITE_CHUNK):
                part = todo[c0:c0 + WRITE_CHUNK]
                recs, off, rows = eng.anib_rows_batch([ids[q] for q, _ in part], [ids[s] for _, s in part], fragsize)
                for k, (q, s) in enumerate(part):
                    results[(q, s)] = _tuple(q, s, recs[k])
                    if s not in subject:
                        r = anim.fasta_records(by_stem[s])
                        subject[s] = ([x[0] for x in r], [x[1] for x in r])
                    f = table_path(outdir, q, s)
                    anib.write_blast_tab(f, rows[int(off[k]):int(off[k + 1])], *subject[s])
                    written.append(f)
        elif todo:
            recs = eng.anib_pairs([ids[q] for q, _ in todo], [ids[s] for _, s in todo], fragsize)
            for (q, s), rec in zip(todo, recs):
                results[(q, s)] = _tuple(q, s, rec)
    finally:
        if scratch_store:
            eng.clear_genomes()
    results = {k: results[k] for k in ((q, s) for q in stems for s in stems if q != s) if k in results}      # the run's pair order, whatever was recovered (a screened run: without the dropped pairs)
    mats = anib.process_blast_results(results, lengths)
    if screened is not None:      # process_blast starts every cell as a perfect match (identity and coverage 1.0, no errors): a pair nobody searched is NaN
        dropped = [(q, s) for q in stems for s in stems if q != s and (q, s) not in results]
        if dropped:
            qi, si = (np.array([stems.index(x[k]) for x in dropped]) for k in (0, 1))
            for name, frame in mats.items():
                v = frame.to_numpy(dtype=np.float64, copy=True)
                v[qi, si] = np.nan
                mats[name] = type(frame)(v, index=frame.index, columns=frame.columns)
    return AnibRun(lengths, fraglengths, results, mats, recovered, written, screened)
