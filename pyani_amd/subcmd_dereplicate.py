"""Dereplicate: one genome per species, by the greedy rule of dRep, galah, skani and CD-HIT.  pyani has no such step.

The genomes are loaded once and screened; then the genomes are walked from the best score to the worst, a genome within the threshold
of an already chosen representative joins one, any other becomes a representative (pyani_amd.screen.representatives_of_pairs is the
statement, Engine.screen_representatives the kernels).  Unlike the connected components of run_anim_components — single linkage, where
a chain a-b-c-d is one component although a and d may be far apart — no two representatives are within the threshold of each other,
and every other genome is within it of its representative.

exact=None: the rule runs on the screen's kept pairs, weight = the shared sampled k-mers.  exact="anim": ONE anim_pairs call aligns the
kept pairs; an undirected pair is an edge iff both ordered comparisons have a result and, in both, identity >= min_ani and the
alignment coverage of the query >= min_coverage (the quantities of run_anim's matrices: identity, aln_length / query length); its
weight is floor(min(identity_ab, identity_ba) * 1e6); the rule runs on that list through the same list entry.

With write_output: `screen_output/screen_pairs.tab` (the screen's kept pairs), `screen_representatives.tab` (one line per
representative: cluster, representative, size, score) and `screen_clusters.tab` (one line per genome: genome, representative, via).

secondary="average" / "complete"  replaces the greedy rule by dRep's SECONDARY CLUSTERING: average- or complete-linkage
hierarchical clustering of the distances inside every connected component, the tree cut at `cutoff`, the member of the greatest score
representing each cluster (pyani_amd.screen.linkage_of_pairs is the statement, Engine.screen_linkage the kernels).  exact=None: the
distance of a pair is 1 minus the smaller of the two directions' screen identities (the numbers of screen_identity.tab), the default
cutoff 1 - screen.min_identity.  exact="anim": an undirected pair carries a distance iff both ordered comparisons have a result and, in
both, coverage >= min_coverage — min_ani does NOT filter, the tree needs the far pairs too —, dist = 1 - min(identity_ab, identity_ba),
the default cutoff 1 - min_ani.  Both defaults are the float64 results of those subtractions, unrounded (1 - 0.95 is
0.050000000000000044).  A pair without a distance sits at 1.0, dRep's ANI 0.  `screen_linkage.tab` is added: one line per merge.

evaluate=True adds dRep's EVALUATE step to either rule: for the clusters the run returns, every genome's centrality
(its mean pair weight to the other members of its cluster, an absent pair counting 0), every cluster's medoid, weakest inside pair and
whether it is a clique, and the cluster each cluster comes closest to (pyani_amd.screen.evaluate_of_pairs is the statement,
Engine.screen_evaluate the kernels).  The list evaluated is the one the clusters come from: the greedy rule's own edges; with secondary=
and exact=None the screen's kept pairs, weight = the shared sampled k-mers; with secondary= and exact="anim" the pairs that carry a
distance, weight = floor(min(identity_ab, identity_ba) * 1e6) (exact_edges with min_ani = 0).  `screen_evaluation_genomes.tab` and
`screen_evaluation_clusters.tab` are added.  winner="medoid" (implies evaluate) makes every cluster's medoid its representative — the
member most central by the pair weights, ties to the greater score — where winner="score", the default, keeps the best-scored member;
the clusters themselves do not change.  dRep's completeness and contamination terms are not computed: pass them through scores=.

OUT OF SCOPE here: ANIb as the exact step, recovery, collective runs, linkage methods other than the two, and distances formed from the
index's shared counts on the device.  Single-process: one engine, or several GPUs of this node (devices / workers).
"""
from pathlib import Path
from typing import Dict, List, Mapping, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib, files, screen as screen_mod
from .engine import Engine, default_engine

EXACT = (None, "anim")
WINNERS = ("score", "medoid")
LINKAGE_FILL = 1.0      # secondary=: the distance of a pair that carries none (ANI 0)


class DereplicateRun(NamedTuple):
    genome_ids: Dict[str, int]                 # stem -> 1-based id in sorted-path order
    lengths: Dict[str, int]
    screened: screen_mod.ScreenedPairs
    records: Optional[np.ndarray]              # exact="anim": the anim_pairs records of the kept pairs, in their order; None otherwise
    edges: Tuple[np.ndarray, np.ndarray, np.ndarray]      # (a, b, weight) the greedy rule ran on: positions in the order of the stems
    clusters: screen_mod.ScreenClusters
    written: List[Path]
    linkage: Optional[screen_mod.ScreenLinkage] = None      # secondary=: the linkage the clusters come from (edges is then (a, b, dist))

    def representatives(self) -> List[str]:
        return self.clusters.representatives()

    @property
    def evaluation(self) -> Optional[screen_mod.ScreenEvaluation]:
        """The evaluation of the clusters: None unless the run was asked for one (EvaluatedDereplicateRun)."""
        return None


class EvaluatedDereplicateRun(DereplicateRun):
    """The DereplicateRun of evaluate=True / winner="medoid": the same eight fields, in the same order, and the ScreenEvaluation of the
    clusters as the attribute `evaluation`.  The tuple itself is unchanged, so that whatever unpacks or compares a DereplicateRun
    keeps working."""
    evaluation = None

    def __new__(cls, *fields, evaluation=None):
        self = super().__new__(cls, *fields)
        self.evaluation = evaluation
        return self


def read_scores(scores) -> Optional[Dict[str, float]]:
    """{stem: score} of `scores`: None, a mapping, or the path of a two-column TSV (stem, score; lines starting with # are skipped)."""
    if scores is None:
        return None
    if isinstance(scores, Mapping):
        return {str(k): v for k, v in scores.items()}
    out: Dict[str, float] = {}
    for no, line in enumerate(Path(scores).read_text().splitlines(), 1):
        if not line.strip() or line.startswith("#"):
            continue
        cols = line.rstrip("\n").split("\t")
        if len(cols) != 2:
            raise ValueError(f"{scores}, line {no}: two tab-separated columns are needed (stem, score)")
        try:
            out[cols[0]] = float(cols[1])
        except ValueError:
            raise ValueError(f"{scores}, line {no}: {cols[1]!r} is no number") from None
    return out


def scores_for(stems: List[str], scores: Optional[Mapping]) -> Optional[np.ndarray]:
    """The scores in the order of the stems (None stays None).  ValueError for a score of an unknown stem, a stem without a score, and
    what screen.score_keys refuses."""
    if scores is None:
        return None
    unknown = sorted(set(scores) - set(stems))
    if unknown:
        raise ValueError(f"a score is given for {unknown[0]!r}, which is no genome of this run")
    missing = [s for s in stems if s not in scores]
    if missing:
        raise ValueError(f"{missing[0]!r} has no score")
    out = np.array([scores[s] for s in stems], dtype=object)
    screen_mod.score_keys(list(out))
    return np.array([float(x) for x in out], dtype=np.float64)


def exact_edges(a, b, recs, length, min_ani: float, min_coverage: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, weight) with a < b of the undirected edges among the ordered pairs (a[e], b[e]) with the anim_pairs records recs[e]
    (a[e] the query, nucmer's reference) and length[v] the genomes' lengths: an edge iff both directions have a result and, in both,
    identity >= min_ani and ref_aln_len / length[query] >= min_coverage; weight = floor(min of the two identities * 1e6)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    status = np.asarray(recs["status"])
    bad = (status != 0) & (status != _lib.PG_ANIM_NO_ALIGNMENT)
    if bad.any():
        raise RuntimeError(f"GPU ANIm comparison failed with status {int(status[bad][0])}")
    ident = np.asarray(recs["identity"], dtype=np.float64)
    cov = np.asarray(recs["ref_aln_len"], dtype=np.float64) / np.asarray(length, dtype=np.float64)[a]
    ok = (status == 0) & (ident >= min_ani) & (cov >= min_coverage)
    good = {(x, y): i for x, y, i, k in zip(a.tolist(), b.tolist(), ident.tolist(), ok.tolist()) if k}
    ea, eb, w = [], [], []
    for (x, y), i in good.items():
        if x < y and (y, x) in good:
            ea.append(x)
            eb.append(y)
            w.append(int(np.floor(min(i, good[(y, x)]) * 1e6)))
    return np.array(ea, dtype=np.int32), np.array(eb, dtype=np.int32), np.array(w, dtype=np.uint32)


def linkage_edges(a, b, recs, length, min_coverage: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, dist) with a < b of the undirected pairs that carry a distance, among the ordered pairs (a[e], b[e]) with the anim_pairs
    records recs[e] (as exact_edges takes them): a pair carries one iff both directions have a result and, in both,
    ref_aln_len / length[query] >= min_coverage; dist = 1 - min of the two identities (float64; an identity above 1 gives 0).  No
    identity threshold: the tree needs the far pairs too."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    status = np.asarray(recs["status"])
    bad = (status != 0) & (status != _lib.PG_ANIM_NO_ALIGNMENT)
    if bad.any():
        raise RuntimeError(f"GPU ANIm comparison failed with status {int(status[bad][0])}")
    ident = np.asarray(recs["identity"], dtype=np.float64)
    cov = np.asarray(recs["ref_aln_len"], dtype=np.float64) / np.asarray(length, dtype=np.float64)[a]
    ok = (status == 0) & (cov >= min_coverage)
    good = {(x, y): i for x, y, i, k in zip(a.tolist(), b.tolist(), ident.tolist(), ok.tolist()) if k}
    ea, eb, d = [], [], []
    for (x, y), i in good.items():
        if x < y and (y, x) in good:
            ea.append(x)
            eb.append(y)
            d.append(max(0.0, 1.0 - min(i, good[(y, x)])))
    return np.array(ea, dtype=np.int32), np.array(eb, dtype=np.int32), np.array(d, dtype=np.float64)


def screen_linkage_edges(screened) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, dist) of a screen's kept pairs as they stand (both directions): dist = 1 - the direction's screen identity
    (ScreenedPairs.identity, the numbers of screen_identity.tab).  The linkage takes the maximum over a pair's entries, which is 1 minus
    the smaller of the two directions' identities."""
    return screened.a, screened.b, np.maximum(0.0, 1.0 - np.asarray(screened.identity(), dtype=np.float64))


def run_dereplicate(indir, outdir=None, screen=None, scores=None, exact: Optional[str] = None, min_ani: float = 0.95, min_coverage: float = 0.1,
                    write_output: bool = False, engine: Optional[Engine] = None, devices: Optional[List[int]] = None,
                    workers: Optional[int] = None, evaluate: bool = False, winner: str = "score", secondary: Optional[str] = None,
                    cutoff: Optional[float] = None) -> DereplicateRun:
    """The greedy representatives of every FASTA file of `indir`.  screen: a ScreenOptions or a bare identity threshold (required: there
    is no default threshold).  scores: None (the sketch sizes: the larger assembly wins), a {stem: score} mapping or the path of a
    two-column TSV; finite and >= 0, greater is better, ties to the genome earlier in sorted-path order.  exact: None or "anim" (see the
    module's text; min_ani and min_coverage matter for "anim" only).  outdir is needed for write_output only; devices / workers: several
    GPUs of this node, ignored when `engine` is given.  secondary: None (the greedy rule), "average" or "complete" (linkage inside every
    component, see the module's text); cutoff: where its trees are cut, None = 1 - min_ani with exact="anim" and 1 - screen.min_identity
    otherwise; it must lie in [0, 1).  evaluate: the clusters are evaluated too (DereplicateRun.evaluation, two more tables; see the
    module's text); winner: "score" (every cluster's best-scored member represents it) or "medoid" (its medoid does; implies evaluate).
    With both at their defaults nothing changes.  Every ValueError is raised before any work is done."""
    if screen is None:
        raise ValueError("run_dereplicate needs screen= (a ScreenOptions or an identity threshold)")
    if write_output and outdir is None:
        raise ValueError("write_output needs an output directory")
    if exact not in EXACT:
        raise ValueError(f"exact must be one of {EXACT}, not {exact!r}")
    if winner not in WINNERS:
        raise ValueError(f"winner must be one of {WINNERS}, not {winner!r}")
    evaluate = bool(evaluate) or winner == "medoid"
    screen = screen_mod.check_options(screen)
    if secondary is None:
        if cutoff is not None:
            raise ValueError("cutoff belongs to secondary= (the greedy rule has none)")
    else:
        if cutoff is None:
            cutoff = 1.0 - (float(min_ani) if exact == "anim" else float(screen.min_identity))
        secondary, cutoff, _ = screen_mod.check_linkage(secondary, cutoff, LINKAGE_FILL)
    paths = files.get_fasta_paths(Path(indir))
    stems = [p.stem for p in paths]
    if len(set(stems)) != len(stems):
        raise ValueError("two input files share a stem (pyani keys every result by Path.stem)")
    given = scores_for(stems, read_scores(scores))
    own = None
    if engine is None and (devices is not None or workers):
        from . import multi
        engine = multi.engine_for(devices, workers)
        own = engine if isinstance(engine, multi.MultiEngine) else None
    try:
        return _run(paths, stems, outdir, screen, given, exact, float(min_ani), float(min_coverage), write_output, engine or default_engine(), secondary, cutoff,
                    evaluate, winner)
    finally:
        if own is not None:
            own.close()


def evaluated_edges(screened, edges, recs, length, exact, min_coverage, secondary) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, b, weight) of the list an evaluation reads: the greedy rule's own edges; under secondary= the screen's kept pairs with weight =
    shared (exact=None), or the pairs that carry a distance with weight = floor(min of the two identities * 1e6) (exact="anim":
    exact_edges without an identity threshold)."""
    if secondary is None:
        return edges
    if exact == "anim":
        return exact_edges(screened.a, screened.b, recs, length, 0.0, min_coverage)
    return screened.a, screened.b, screened.shared


def _run(paths, stems, outdir, screen, given, exact, min_ani, min_coverage, write_output, eng, secondary=None, cutoff=None, evaluate=False,
         winner="score") -> DereplicateRun:
    genome_ids = {s: k + 1 for k, s in enumerate(stems)}
    scratch_store = eng.genome_count() == 0
    lengths: Dict[str, int] = {}
    recs = None
    try:
        ids = np.zeros(len(paths), dtype=np.int64)
        for k, (p, (gid, total, _)) in enumerate(zip(paths, eng.add_fasta_batch(paths))):
            ids[k], lengths[p.stem] = gid, total
        screened = eng.screen_candidates(ids.tolist(), screen, labels=stems)
        n = len(stems)
        score = screen_mod.score_keys(given, screened.sizes)
        edges = (screened.a, screened.b, screened.shared)
        if exact == "anim":
            recs = np.zeros(0, dtype=Engine.ANIM_DTYPE)
            if len(screened.a):      # the query is nucmer's reference, as in run_anim
                recs = eng.anim_pairs(ids[screened.a], ids[screened.b])
            if secondary is None:
                edges = exact_edges(screened.a, screened.b, recs, [lengths[s] for s in stems], min_ani, min_coverage)
            else:
                edges = linkage_edges(screened.a, screened.b, recs, [lengths[s] for s in stems], min_coverage)
        elif secondary is not None:
            edges = screen_linkage_edges(screened)
        nodes = measured = None
        try:
            if n and secondary is None:
                rep, via = eng.screen_representatives(*edges, n=n, score=score)
            elif n:
                nodes = eng.screen_linkage(*edges, n=n, score=score, method=secondary, cutoff=cutoff, fill=LINKAGE_FILL)
            else:
                rep, via = np.zeros(0, np.int32), np.zeros(0, np.uint32)
                nodes = (rep, rep, rep, np.zeros((0, 4))) if secondary is not None else None
            if evaluate and n:
                measured = eng.screen_evaluate(*evaluated_edges(screened, edges, recs, [lengths[s] for s in stems], exact, min_coverage, secondary), n=n,
                                               label=rep if secondary is None else nodes[2], score=score)
        finally:
            if secondary is None:
                eng.screen_representatives_release()
            else:
                eng.screen_linkage_release()
            if evaluate:
                eng.screen_evaluate_release()
    finally:
        if scratch_store:
            eng.clear_genomes()
    linkage = None
    if secondary is None:
        clusters = screen_mod.clusters_from_nodes(stems, rep, via, score)
    else:
        linkage = screen_mod.linkage_from_nodes(stems, *nodes[:3], score, nodes[3], secondary, cutoff, LINKAGE_FILL)
        clusters = linkage.clusters()
    evaluation = None
    if evaluate:
        if measured is None:
            measured = ([np.zeros(0)] * 7, [np.zeros(0)] * 7)
        evaluation = screen_mod.evaluation_from_nodes(stems, clusters.rep, score, *measured)
        if winner == "medoid":
            clusters = evaluation.recentred()
    written: List[Path] = []
    if write_output:
        from .subcmd_screen import tab_path, write_pairs_tab
        written = [write_pairs_tab(outdir, screened), tab_path(outdir, "representatives"), tab_path(outdir, "clusters")]
        clusters.frame().to_csv(written[1], index=False, sep="\t")
        clusters.membership_frame().to_csv(written[2], index=False, sep="\t")
        if linkage is not None:
            written.append(tab_path(outdir, "linkage"))
            write_linkage_tab(written[3], linkage)
        if evaluation is not None:
            written += [tab_path(outdir, "evaluation_genomes"), tab_path(outdir, "evaluation_clusters")]
            write_evaluation_tabs(written[-2], written[-1], evaluation)
    run = DereplicateRun(genome_ids, lengths, screened, recs, edges, clusters, written, linkage)
    return run if evaluation is None else EvaluatedDereplicateRun(*run, evaluation=evaluation)


def write_evaluation_tabs(genomes_path, clusters_path, evaluation) -> None:
    """`screen_evaluation_genomes.tab` (ScreenEvaluation.genome_frame) and `screen_evaluation_clusters.tab` (.cluster_frame); the floats
    with repr's precision, so that float(text) gives the bits back."""
    for path, t in ((genomes_path, evaluation.genome_frame()), (clusters_path, evaluation.cluster_frame())):
        floats = [c for c in t.columns if t[c].dtype == np.float64]
        t = t.astype({c: object for c in floats})
        for c in floats:
            t[c] = [repr(float(x)) for x in t[c]]
        t.to_csv(path, index=False, sep="\t")


def read_evaluation_tab(path):
    """A table of write_evaluation_tabs as a DataFrame (names as text, an absent name as ""; the floats parsed to the bits written)."""
    import pandas as pd
    return pd.read_csv(path, sep="\t", keep_default_na=False, float_precision="round_trip")


def write_linkage_tab(path, linkage) -> None:
    """`screen_linkage.tab`: one line per merge — component, left, right, height, size in scipy's numbering (ScreenLinkage.merges_frame),
    the heights with repr's precision, so that float(text) gives the bits back."""
    t = linkage.merges_frame()
    with open(path, "w") as out:
        out.write("component\tleft\tright\theight\tsize\n")
        for c, x, y, h, s in zip(t["component"], t["left"], t["right"], t["height"], t["size"]):
            out.write(f"{c}\t{x}\t{y}\t{float(h)!r}\t{s}\n")


def read_linkage_tab(path) -> List[Tuple[str, int, int, float, int]]:
    """The lines of a `screen_linkage.tab` as (component, left, right, height, size)."""
    rows = []
    for line in Path(path).read_text().splitlines()[1:]:
        c, x, y, h, s = line.split("\t")
        rows.append((c, int(x), int(y), float(h), int(s)))
    return rows
