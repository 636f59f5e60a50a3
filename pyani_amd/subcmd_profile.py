"""The screen's profile over a collection and a partition of it: what the genomes of every cluster SHARE.  After a
dereplication one asks how large a cluster's core is and how much of it each member carries (the k-mer proxy for completeness), which
genomes carry material their own cluster lacks but other clusters have (the contamination / transfer proxy), and which k-mers are
diagnostic for a cluster — in (nearly) every member and in no other genome: where primer and probe design starts.  The collection is
indexed once (Engine.screen_search_index: every distinct sampled k-mer with its holders, resident on the device) and
Engine.screen_search_profile reads the answers off the index; the index never leaves the device.

The collection comes from FASTA files (`db_dir`, optionally db_batch files at a time) or from a saved search index (`index`), exactly as
run_screen_search takes it.  The partition comes from `partition=` — a mapping stem -> cluster name, or a table whose first two columns
are genome and cluster name (a header line `genome<TAB>...` is skipped): `screen_clusters.tab` of run_dereplicate is one — or from
`classes=`, pyani's classes.txt (hash, stem, class).  A cluster's naming node is its first member in column order.

Every count is of SAMPLED k-mers: at scale s a marker count estimates 1 / s of the count over all k-mers; scale=1 gives all of them.
With write_output, under `<outdir>/screen_output/`: profile_genomes.tab, profile_clusters.tab, profile_spectrum.tab (cluster, occupancy,
k-mers; zero rows omitted) and profile_markers.tab (cluster, the k-mer as text, occupancy).  A single Engine only.
"""
from pathlib import Path
from typing import Dict, List, NamedTuple, Optional

import numpy as np

from . import files, screen as screen_mod
from .engine import Engine, default_engine
from .subcmd_screen import OUTDIR
from .subcmd_search import _stems, load_db
from .subcmd_searchdb import _check_batch, _check_engine

TABLES = ("genomes", "clusters", "spectrum", "markers")


class ProfileRun(NamedTuple):
    profile: screen_mod.ScreenProfile      # labels = the stems
    cluster_names: List[str]                # the partition's own name of every cluster, in cluster order
    written: List[Path]                     # the four tables, in the order of TABLES ([] without write_output)


def profile_tab_path(outdir, name: str) -> Path:
    return Path(outdir) / OUTDIR / f"profile_{name}.tab"


def read_partition(partition) -> Dict[str, str]:
    """stem -> cluster name of partition=: a mapping as it is, or the first two tab-separated columns of a table (empty lines, lines that
    begin with # and a header line whose first field is `genome` are skipped).  ValueError for a line of one field, a stem without a
    cluster name and a stem given twice."""
    if isinstance(partition, dict):
        pairs = [(str(k), v) for k, v in partition.items()]
    else:
        pairs = []
        for no, line in enumerate(Path(partition).read_text().splitlines(), 1):
            if not line.strip() or line.startswith("#"):
                continue
            fields = line.split("\t")
            if no == 1 and fields[0] == "genome":
                continue
            if len(fields) < 2:
                raise ValueError(f"{partition}: line {no} has no cluster column (genome<TAB>cluster)")
            pairs.append((fields[0].strip(), fields[1]))
    return _named(pairs, "partition")


def read_classes(classes) -> Dict[str, str]:
    """stem -> class of pyani's classes.txt: hash<TAB>stem<TAB>class per line.  ValueErrors as read_partition's."""
    pairs = []
    for no, line in enumerate(Path(classes).read_text().splitlines(), 1):
        if not line.strip() or line.startswith("#"):
            continue
        fields = line.split("\t")
        if len(fields) < 2:
            raise ValueError(f"{classes}: line {no} is not hash<TAB>stem<TAB>class")
        pairs.append((fields[1].strip(), fields[2] if len(fields) > 2 else None))
    return _named(pairs, "classes")


def _named(pairs, what: str) -> Dict[str, str]:
    out: Dict[str, str] = {}
    for stem, name in pairs:
        if stem in out:
            raise ValueError(f"{what}: the genome {stem!r} is given twice")
        if name is None or not str(name).strip():
            raise ValueError(f"{what}: the genome {stem!r} has no class")
        out[stem] = str(name).strip()
    return out


def partition_labels(stems, named: Dict[str, str]):
    """(label int32[n], the clusters' names in cluster order) of the stems in column order under stem -> cluster name: a cluster's naming
    node is its first member in column order.  ValueError for a stem the mapping does not know and for one the collection does not hold."""
    held = set(stems)
    unknown = [s for s in named if s not in held]
    if unknown:
        raise ValueError(f"the collection holds no genome {unknown[0]!r}")
    missing = [s for s in stems if s not in named]
    if missing:
        raise ValueError(f"the genome {missing[0]!r} has no class")
    first: Dict[str, int] = {}
    label = np.zeros(len(stems), dtype=np.int32)
    for v, s in enumerate(stems):
        label[v] = first.setdefault(named[s], v)
    return label, list(first)      # (a dict keeps the order of insertion: ascending naming node)


def run_screen_profile(db_dir=None, index=None, partition=None, classes=None, outdir=None, core: float = 0.95, shell: float = 0.15,
                       marker_min_size: int = 2, kmer: int = screen_mod.DEFAULT_KMER, scale: int = screen_mod.DEFAULT_SCALE,
                       db_batch: Optional[int] = None, write_output: bool = True, engine: Optional[Engine] = None) -> ProfileRun:
    """The profile of the collection of `db_dir` (kmer, scale, db_batch as run_screen_search) or of the saved search index `index` (its own
    kmer and scale) under the partition of `partition=` or `classes=` (the module's text).  Everything that can be refused from the
    arguments and the files' names is a ValueError before any device work: neither or both of the two, neither or both of db_dir and
    index, an unknown stem, a stem given twice, a stem without a class, fractions outside 0 < shell <= core <= 1.  The engine holds
    neither a search index nor a profile when this returns (released on errors too)."""
    if (partition is None) == (classes is None):
        raise ValueError("a partition is needed: partition= or classes=, one of them")
    if (db_dir is None) == (index is None):
        raise ValueError("a collection is needed: db_dir= or index=, one of them")
    if index is not None and db_batch is not None:
        raise ValueError("index= reads no file of a collection: db_batch= goes with db_dir")
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")
    _check_engine(engine)
    db_batch = _check_batch(db_batch)
    screen_mod.profile_thresholds([1], core, shell)      # (the fractions, before any work)
    if isinstance(marker_min_size, (bool, float)) or int(marker_min_size) < 1:
        raise ValueError(f"marker_min_size is an integer >= 1, not {marker_min_size!r}")
    named = read_partition(partition) if partition is not None else read_classes(classes)
    if index is None:
        kmer, scale = screen_mod.check_params(kmer, scale)
        db_paths = files.get_fasta_paths(Path(db_dir))
        stems, f = _stems(db_paths, "db"), None
    else:
        f = screen_mod.read_search_index(index)
        stems = list(f.labels)
    label, names = partition_labels(stems, named)
    if not stems:
        raise ValueError("a profile needs a genome")
    eng = engine or default_engine()
    scratch_store = eng.genome_count() == 0
    if db_batch is not None and not scratch_store:
        raise ValueError("db_batch clears the genome store after every batch: it needs an engine whose store is empty")
    try:
        if f is None:
            load_db(eng, db_paths, stems, screen_mod.ScreenOptions(1.0, kmer, scale, screen_mod.DEFAULT_MIN_SHARED), db_batch, {})
        else:
            eng.screen_search_index_adopt(f, str(index))
        profile = eng.screen_search_profile(label, core, shell, marker_min_size)
    finally:
        eng.screen_search_profile_release()
        eng.screen_search_index_release()
        if scratch_store:
            eng.clear_genomes()
    written: List[Path] = []
    if write_output:
        (Path(outdir) / OUTDIR).mkdir(parents=True, exist_ok=True)
        frames = (profile.genome_frame(), profile.cluster_frame(), profile.spectrum_frame(), profile.markers_frame())
        for name, frame in zip(TABLES, frames):
            frame.to_csv(profile_tab_path(outdir, name), index=False, sep="\t")
            written.append(profile_tab_path(outdir, name))
    return ProfileRun(profile, names, written)
