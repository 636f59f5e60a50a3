"""classify — pyani's clique sweep over identity thresholds (pyani/pyani_classify.py:61-165 and trimmed_graph_sequence,
pyani/scripts/subcommands/subcmd_classify.py:122-171) on the GPU.

A graph whose nodes are genomes and whose edges are comparisons above a coverage and an identity floor is trimmed at a rising
identity threshold; every step reports (n_nodes, number of connected components, "every component is a clique").  The reference
walks one networkx graph through the thresholds; here the host derives the list of thresholds (`break_thresholds`, pure numpy)
and the device evaluates all steps at once (pg_classify_edges / pg_classify_sweep: one workgroup per step).  The sequence of
(interval, n_nodes, n_subgraphs, all_k_complete) is the reference's, floats bit for bit, its quirks included:

  * edge weight = Python's min(M[col i][row j], M[col j][row i]) for identity and coverage, in that argument order (NaN rule);
  * the node set is every edge endpoint plus every label EXCEPT THE LAST (pyani_classify.py:108);
  * `min_id or lowest edge` / `max_id or 1`: None and 0 both fall through; with a falsy min_id the lowest edge(s) go before the first
    step, and no edge at all raises IndexError;
  * fewer remaining edges than 1 / resolution: one break per edge (duplicates kept); else numpy.arange(start, stop, resolution);
  * every step is analysed BEFORE its break's edges are removed; a last step at interval 1 follows, analysed after removal.

networkx is not needed: a step's graph is returned as `membership`, a label -> component-representative mapping.
There is no CPU fallback: without a device `classify` raises PyaniGpuError."""
import io
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import pandas as pd

from .engine import Engine, default_engine

LABEL_SLICE_BYTES = 32 << 20      # per-step labels are fetched in slices of at most this many bytes per sweep call


class Cliquesinfo(NamedTuple):
    """Summary of clique structure (pyani_classify.Cliquesinfo)."""
    n_nodes: int
    n_subgraphs: int
    all_k_complete: bool


class SubgraphData(NamedTuple):
    """One step of the sweep (subcmd_classify.SubgraphData, with `membership` in place of the nx.Graph)."""
    interval: float                          # the trimming threshold of this step
    cliqueinfo: Cliquesinfo
    membership: Optional[Dict[object, object]]   # label -> label of the smallest-index member of its component; None if not asked for


def break_thresholds(sorted_edge_identities, min_id=None, max_id=None, resolution: float = 1e-4) -> Tuple[list, np.ndarray]:
    """(intervals, theta) of the sweep from the ascending edge identities (remove_low_weight_edges, pyani_classify.py:160-165, and
    trimmed_graph_sequence, subcmd_classify.py:144-171).  intervals: what each step reports (the breaks, then 1); theta (float64,
    one per step, non-decreasing): step k sees exactly the edges with identity > theta[k].  Host only, no GPU needed."""
    ids = np.ascontiguousarray(sorted_edge_identities, dtype=np.float64)
    if len(ids) > 1 and not (ids[1:] >= ids[:-1]).all():
        raise ValueError("edge identities must be sorted ascending")
    if not min_id and len(ids) == 0:
        raise IndexError("list index out of range")      # the reference's edgelist[0] on a graph without edges
    t0 = min_id or ids[0]
    rest = ids[np.searchsorted(ids, t0, side="right"):]      # edges <= t0 go before the first step
    if len(rest) < 1 / resolution:
        breaks = rest.copy()
    else:
        breaks = np.arange(min_id or rest[0], max_id or 1, resolution)
    theta = np.maximum.accumulate(np.concatenate(([float(t0)], np.asarray(breaks, dtype=np.float64))))
    theta[-1] = max(theta[-1], 1.0)      # the last step: edges <= 1 removed from what is left, then analysed
    return breaks.tolist() + [1], theta


def _matrices(identity, coverage, labels):
    """(I, C, labels): float64 arrays with rows and columns in the coverage frame's column order (the reference walks
    mat_coverage.columns and addresses both frames by label)."""
    if isinstance(coverage, pd.DataFrame):
        cols = list(coverage.columns)
        if len(set(cols)) != len(cols):
            raise ValueError("duplicate labels in the coverage matrix")
        coverage = coverage.loc[cols, cols]
        if isinstance(identity, pd.DataFrame):
            identity = identity.loc[cols, cols]
        labels = cols if labels is None else list(labels)
    elif isinstance(identity, pd.DataFrame):
        raise TypeError("identity and coverage must both be DataFrames or both be arrays")
    I = np.ascontiguousarray(np.asarray(identity, dtype=np.float64))
    C = np.ascontiguousarray(np.asarray(coverage, dtype=np.float64))
    if I.ndim != 2 or I.shape[0] != I.shape[1] or I.shape != C.shape:
        raise ValueError(f"identity {I.shape} and coverage {C.shape} must be square matrices of one size")
    labels = list(range(len(I))) if labels is None else list(labels)
    if len(labels) != len(I):
        raise ValueError("one label per row / column is needed")
    return I, C, labels


def classify(identity, coverage, labels: Optional[Sequence] = None, cov_min: float = 0.5, id_min: float = 0.8, min_id=None, max_id=None,
             resolution: float = 1e-4, memberships: str = "special", engine: Optional[Engine] = None) -> List[SubgraphData]:
    """The whole sequence trimmed_graph_sequence yields for the graph build_graph_from_results makes of the two matrices (defaults:
    scripts/parsers/classify_parser.py).  memberships: "none", "special" (the steps whose components are all cliques, the ones
    subcmd_classify reports) or "all"."""
    if memberships not in ("none", "special", "all"):
        raise ValueError('memberships must be "none", "special" or "all"')
    I, C, labels = _matrices(identity, coverage, labels)
    eng = engine or default_engine()
    n = len(labels)
    n_edges, n_nodes = eng.classify_edges(I, C, id_min=id_min, cov_min=cov_min)
    try:
        ids = np.sort(eng.classify_edge_identities(n_edges))
        intervals, theta = break_thresholds(ids, min_id, max_id, resolution)
        n_sub, complete, _ = eng.classify_sweep(theta)
        want = {"none": np.zeros(0, dtype=np.int64), "special": np.flatnonzero(complete), "all": np.arange(len(theta))}[memberships]
        member: Dict[int, Dict] = {}
        per_call = max(1, LABEL_SLICE_BYTES // (4 * n))
        lab = np.asarray(labels, dtype=object)
        for a in range(0, len(want), per_call):
            steps = want[a:a + per_call]
            _, _, rows = eng.classify_sweep(theta[steps], labels=True)      # any sub-list of theta gives the same per-step answers
            for k, row in zip(steps, rows):
                inside = row >= 0
                member[int(k)] = dict(zip(lab[inside].tolist(), lab[row[inside]].tolist()))
    finally:
        eng.classify_release()
    return [SubgraphData(iv, Cliquesinfo(n_nodes, int(s), bool(c)), member.get(k))
            for k, (iv, s, c) in enumerate(zip(intervals, n_sub, complete))]


def classify_run(run, label_dict: Optional[Dict[str, str]] = None, **kw) -> List[SubgraphData]:
    """classify() for a finished run: an AnimRun (pyani_amd.subcmd_anim) or its `json` dict of Run.df_* strings.  As
    build_graph_from_results (pyani_classify.py:78-79) it PARSES df_identity / df_coverage with pandas.read_json — the reference
    classifies the stored strings, and the parse is not exact to the last bit — and labels them as label_results_matrix does
    (pyani_tools.py:303-320): "<label>:<genome id>", "Genome_id:<genome id>" where label_dict has no entry."""
    js = run if isinstance(run, dict) else run.json
    labels = label_dict or {}

    def frame(text):
        m = pd.read_json(io.StringIO(text))
        m.columns = [f"{labels.get(str(g), 'Genome_id')}:{g}" for g in m.columns]
        m.index = [f"{labels.get(str(g), 'Genome_id')}:{g}" for g in m.index]
        return m

    return classify(frame(js["df_identity"]), frame(js["df_coverage"]), **kw)


def special_intervals(seq: Iterable[SubgraphData]) -> List[SubgraphData]:
    """The steps at which every component is a clique (subcmd_classify.py:109)."""
    return [s for s in seq if s.cliqueinfo.all_k_complete]


def write_classify_tab(path, seq: Iterable[SubgraphData]) -> None:
    """One tab-separated line per step: interval, n_nodes, n_subgraphs, all_k_complete, under a header line.  The reference only
    LOGS these values (subcmd_classify.py:110-116); this file format is this package's own."""
    with open(path, "w") as fh:
        fh.write("interval\tn_nodes\tn_subgraphs\tall_k_complete\n")
        for s in seq:
            fh.write(f"{s.interval!r}\t{s.cliqueinfo.n_nodes}\t{s.cliqueinfo.n_subgraphs}\t{s.cliqueinfo.all_k_complete}\n")
