"""The screen over a directory of FASTA files: the driver of pyani_amd.screen, in the shape of the other run_* drivers.  pyani has no
such subcommand — this is the front end a caller puts before run_anim / run_anib on a large collection: every file of `indir` in sorted
order, ONE engine call for all of them, and the result as labelled frames.  No CLI and no database.

With write_output the frames go to `<outdir>/screen_output/screen_{shared,containment,identity}.tab` in the shape of the legacy
matrix files (tab-separated, labels on both axes).  These are the screen's OWN files: an estimate, never merged into an ANIm or ANIb result.
With min_identity the kept pairs go to `screen_pairs.tab`, and with components=True their connected components to
`screen_components.tab` and `screen_membership.tab`.  With sweep=identities their components at every identity of a ladder
 go to `screen_sweep.tab`.
Single-process: one engine, or several GPUs of this node through pyani_amd.multi.MultiEngine (devices / workers).
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

from . import files, screen
from .engine import Engine, default_engine

OUTDIR = "screen_output"
TAB_NAMES = ("shared", "containment", "identity")


class ScreenRun(NamedTuple):
    lengths: Dict[str, int]          # stem -> genome length, file order
    result: Optional[screen.ScreenResult]      # labels = the stems, file order; None above screen.DENSE_MAX_GENOMES (no dense frames exist)
    screened: Optional[screen.ScreenedPairs] = None      # the kept pairs (min_identity=...), None without
    components: Optional[screen.ScreenComponents] = None      # their connected components (components=True), None without
    sweep: Optional[screen.ScreenSweep] = None      # the components over a ladder of identities (sweep=identities), None without


def tab_path(outdir, name: str) -> Path:
    return Path(outdir) / OUTDIR / f"screen_{name}.tab"


def write_tabs(outdir, result: screen.ScreenResult) -> List[Path]:
    (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
    frames = {"shared": result.shared_frame(), "containment": result.containment(), "identity": result.identity()}
    out = []
    for name in TAB_NAMES:
        frames[name].to_csv(tab_path(outdir, name), index=True, sep="\t")
        out.append(tab_path(outdir, name))
    return out


def write_pairs_tab(outdir, screened: screen.ScreenedPairs) -> Path:
    """`<outdir>/screen_output/screen_pairs.tab` of a screened run: one line per kept pair — query, subject, shared, containment,
    identity — in the order of the selection."""
    (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
    screened.frame().to_csv(tab_path(outdir, "pairs"), index=False, sep="\t")
    return tab_path(outdir, "pairs")


def write_components_tabs(outdir, components: screen.ScreenComponents) -> List[Path]:
    """`<outdir>/screen_output/screen_components.tab` — one line per component: component, size, representative, edges, complete — and
    `screen_membership.tab` — one line per genome: genome, component, representative."""
    (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
    components.frame().to_csv(tab_path(outdir, "components"), index=False, sep="\t")
    components.membership_frame().to_csv(tab_path(outdir, "membership"), index=False, sep="\t")
    return [tab_path(outdir, "components"), tab_path(outdir, "membership")]


def write_sweep_tab(outdir, sweep: screen.ScreenSweep) -> Path:
    """`<outdir>/screen_output/screen_sweep.tab`: one line per step of the ladder — step, identity, entries, components, singletons,
    largest, pair_slots, complete (ScreenSweep.frame; the identity in its shortest digits that read back to the same float)."""
    (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
    sweep.frame().to_csv(tab_path(outdir, "sweep"), index=False, sep="\t")
    return tab_path(outdir, "sweep")


def run_screen(indir, outdir=None, kmerSize: int = screen.DEFAULT_KMER, scale: int = screen.DEFAULT_SCALE, write_output: bool = False,
               engine: Optional[Engine] = None, devices: Optional[List[int]] = None, workers: Optional[int] = None,
               min_identity: Optional[float] = None, components: bool = False, sweep=None) -> ScreenRun:
    """The screen over every FASTA file of `indir`.  outdir is needed for write_output only.
    devices / workers: run on several GPUs of this node (pyani_amd/multi.py); ignored when `engine` is given.
    min_identity: when given, the pairs whose identity estimate reaches it are selected on the device (Engine.screen_candidates,
    ScreenRun.screened) and written to screen_pairs.tab with write_output.  More than screen.DENSE_MAX_GENOMES files have no dense frames:
    `result` is None, only the kept pairs exist, and a call without min_identity raises ValueError.
    components: with True (it needs min_identity) the connected components of the kept pairs are worked out on the device too
    (ScreenedPairs.components; ScreenRun.components) and written to screen_components.tab and screen_membership.tab with
    write_output.  The default leaves the run as it was.
    sweep: a ladder of strictly ascending identities (at most 4096).  The components of the kept pairs at EVERY step are worked out in
    one pass on the device (Engine.screen_sweep_of; ScreenRun.sweep) and written to screen_sweep.tab with write_output.
    It stands beside min_identity and needs none: its pairs are those kept at the ladder's first identity.  A single engine only
    (ValueError with devices / workers that give several).  The default None does and writes nothing new."""
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")     # before any work is done
    if components and min_identity is None:
        raise ValueError("components=True needs min_identity: the components are those of the kept pairs")
    kmerSize, scale = screen.check_params(kmerSize, scale)
    if sweep is not None:
        sweep = screen.check_ladder(sweep)      # before any work is done
    if min_identity is not None:
        min_identity = screen.check_options(screen.ScreenOptions(min_identity, kmerSize, scale)).min_identity
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        return _run_screen(indir, outdir, kmerSize, scale, write_output, engine or default_engine(), min_identity, components, sweep)
    finally:
        if own is not None:
            own.close()


def _run_screen(indir, outdir, kmerSize, scale, write_output, eng, min_identity=None, components=False, sweep=None) -> ScreenRun:
    if sweep is not None and not hasattr(eng, "screen_sweep_of"):      # before any work is done
        raise ValueError("sweep= runs on a single engine (DESIGN.md §16.10)")
    paths = files.get_fasta_paths(Path(indir))
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError("two input files share a stem (pyani keys every result by Path.stem)")
    dense = len(paths) <= screen.DENSE_MAX_GENOMES
    if not dense and min_identity is None and sweep is None:      # before any work is done
        raise ValueError(f"{len(paths)} genomes are more than the {screen.DENSE_MAX_GENOMES} a dense screen matrix takes: "
                         "pass min_identity to get the kept pairs instead (ScreenRun.screened), or sweep")
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    try:
        ids = []
        for p, (gid, total, _) in zip(paths, eng.add_fasta_batch(paths)):
            ids.append(gid)
            lengths[p.stem] = total
        result = screen.screen_genomes(eng, ids, stems, kmerSize, scale) if dense else None
        screened = None
        if min_identity is not None:
            screened = eng.screen_candidates(ids, screen.ScreenOptions(min_identity, kmerSize, scale), labels=stems)
        comps = None
        if components:
            try:
                comps = screened.components(engine=eng)
            finally:
                eng.screen_components_release()
        swept = None
        if sweep is not None:
            swept = eng.screen_sweep_of(ids, screen.ScreenOptions(float(sweep[0]), kmerSize, scale), sweep, labels=stems)
    finally:
        if scratch_store:
            eng.clear_genomes()
    if write_output:
        if result is not None:
            write_tabs(outdir, result)
        if screened is not None:
            write_pairs_tab(outdir, screened)
        if comps is not None:
            write_components_tabs(outdir, comps)
        if swept is not None:
            write_sweep_tab(outdir, swept)
    return ScreenRun(lengths, result, screened, comps, swept)
