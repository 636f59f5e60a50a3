"""ANIm per connected component of the screen's kept pairs: the driver behind the screen for collections that no n x n frame can hold
(DESIGN.md §16.3).  pyani has no such step; this is the primary clustering of dRep or skani put in front of pyani's ANIm.

A component is closed under the screen's rule — every kept pair lies inside one, and no exact comparison is wanted across two — so a
collection of any size falls apart into pieces that each fit the machinery of run_anim: the genomes are loaded once, the screen gives
the kept pairs and their components, ONE anim_pairs call aligns all kept pairs (built from the ScreenedPairs arrays, never from
permutations of the stems), and the results are assembled PER COMPONENT of two or more members, over that component's members only:
the five NaN-initialised frames, the Comparison rows and the JSON strings of run_anim, of the component's size.  A component of more
than MATRIX_MAX_GENOMES members keeps its results and rows and has no frames; a singleton is only listed.

With write_output the three screen tables are written (`screen_output/screen_pairs.tab`, `screen_components.tab`,
`screen_membership.tab`).  OUT OF SCOPE here: an ANIb variant, alignment files (.filter / .delta), recovery, collective runs, and
components fed from the dense resident selection without reading the pairs back (the dense path reads them once; the index path of
Engine.screen_components_of reads none).  Single-process: one engine, or several GPUs of this node (devices / workers).
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import pandas as pd

from . import anim, files, screen as screen_mod
from .engine import Engine, default_engine

MATRIX_MAX_GENOMES = 8192      # members of a component that still gets its five frames


class ComponentRun(NamedTuple):
    """One component of two or more members, in the shape of subcmd_anim.AnimRun less its files."""
    members: List[str]                                           # stems, in the order of the run
    representative: str
    genome_ids: Dict[str, int]                                   # stem -> genome id of the WHOLE run (1-based, sorted-path order)
    lengths: Dict[str, int]
    results: Dict[Tuple[str, str], Tuple[int, int, float, int]]  # (query stem, subject stem) -> parse_delta tuple
    comparisons: List[dict]
    matrices: Optional[Dict[str, pd.DataFrame]]                  # None beyond MATRIX_MAX_GENOMES members
    json: Optional[Dict[str, str]]


class AnimComponentsRun(NamedTuple):
    genome_ids: Dict[str, int]
    lengths: Dict[str, int]
    screened: screen_mod.ScreenedPairs
    components: screen_mod.ScreenComponents
    runs: Dict[int, ComponentRun]                                # component number -> its run; singletons have none
    written: List[Path]


def run_anim_components(indir, outdir=None, screen=None, nofilter: bool = False, maxmatch: bool = False, skip_zero: bool = False,
                        write_output: bool = False, engine: Optional[Engine] = None, devices: Optional[List[int]] = None,
                        workers: Optional[int] = None) -> AnimComponentsRun:
    """ANIm over the kept pairs of every FASTA file of `indir`, assembled per component.  screen: a ScreenOptions or a bare identity
    threshold (required: there is no default threshold).  nofilter / maxmatch / skip_zero as run_anim; outdir is needed for write_output
    only; devices / workers: several GPUs of this node, ignored when `engine` is given."""
    if screen is None:
        raise ValueError("run_anim_components needs screen= (a ScreenOptions or an identity threshold)")
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")     # before any work is done
    screen = screen_mod.check_options(screen)
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        return _run(indir, outdir, screen, nofilter, maxmatch, skip_zero, write_output, engine or default_engine())
    finally:
        if own is not None:
            own.close()


def _run(indir, outdir, screen, nofilter, maxmatch, skip_zero, write_output, eng) -> AnimComponentsRun:
    paths = files.get_fasta_paths(Path(indir))
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError("two input files share a stem (pyani keys every result by Path.stem)")
    genome_ids = {s: k + 1 for k, s in enumerate(stems)}
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    try:
        ids = np.zeros(len(paths), dtype=np.int64)
        for k, (p, (gid, total, _)) in enumerate(zip(paths, eng.add_fasta_batch(paths))):
            ids[k], lengths[p.stem] = gid, total
        screened = eng.screen_candidates(ids.tolist(), screen, labels=stems)
        try:
            comps = screened.components(engine=eng)
        finally:
            eng.screen_components_release()
        recs = None
        if len(screened.a):      # the query is nucmer's reference, as in run_anim
            recs = eng.anim_pairs(ids[screened.a], ids[screened.b], filter_1to1=not nofilter, maxmatch=maxmatch)
    finally:
        if scratch_store:
            eng.clear_genomes()
    # every kept pair lies inside one component: its results go to the component of its query
    per: Dict[int, Dict[Tuple[str, str], Tuple[int, int, float, int]]] = {int(c): {} for c in np.flatnonzero(comps.size >= 2)}
    if recs is not None:
        for a, b, c, rec in zip(screened.a.tolist(), screened.b.tolist(), comps.component[screened.a].tolist(), recs):
            try:
                per[c][(stems[a], stems[b])] = anim._tuple(rec)
            except ZeroDivisionError:
                if not skip_zero:
                    raise
    runs: Dict[int, ComponentRun] = {}
    for c, results in per.items():
        members = [stems[v] for v in comps.members(c).tolist()]
        sub_len = {s: lengths[s] for s in members}
        sub_ids = {s: genome_ids[s] for s in members}
        mats = anim.assemble_run_matrices(results, sub_len, genome_ids=sub_ids) if len(members) <= MATRIX_MAX_GENOMES else None
        runs[c] = ComponentRun(members, stems[int(comps.representative[c])], sub_ids, sub_len, results,
                               anim.comparison_rows(results, sub_len, sub_ids, maxmatch=maxmatch), mats,
                               None if mats is None else anim.run_matrices_to_json(mats))
    written: List[Path] = []
    if write_output:
        from .subcmd_screen import write_components_tabs, write_pairs_tab
        written = [write_pairs_tab(outdir, screened)] + write_components_tabs(outdir, comps)
    return AnimComponentsRun(genome_ids, lengths, screened, comps, runs, written)
