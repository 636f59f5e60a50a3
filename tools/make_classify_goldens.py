#!/usr/bin/env python3
"""Generate tests/golden/classify/*.json.gz by running the REAL reference's classify code on the cases of tests/classify_cases.py.

Runs only where the reference tree exists (a checkout beside this repository, or $PYANI_REFERENCE).  It imports the reference's
pyani.pyani_classify as part of its package (tools/bio_shim stands in for absent third-party imports, as in tools/make_goldens.py) and loads
scripts/subcommands/subcmd_classify.py by file path (its package __init__ pulls in Biopython's Entrez).  To hand the reference exact
float64 matrices, the `pd` name inside the reference module is replaced for the duration of a call by a stand-in whose read_json
returns the prepared DataFrame; the case marked json=True goes through real DataFrame.to_json() strings and the unmodified read_json.

Per case the golden holds: the parameters, the inputs (hex of the float64 bytes up to 60 genomes, else the generator arguments) with
the sha1 of their bytes, the labels, every tuple (interval, n_nodes, n_subgraphs, all_k_complete) the reference emits, its wall times,
and up to 400 genomes the partition at every step (networkx.connected_components, as lists of node indices into `labels`).
DATA only — no reference source text is written anywhere.

Usage: python tools/make_classify_goldens.py [case ...]"""
import gzip
import importlib.util
import json
import os
import sys
import time
import types
from argparse import Namespace
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("PYANI_REFERENCE", ROOT.parent / "reference"))      # a checkout of the reference beside this repository
OUT = ROOT / "tests" / "golden" / "classify"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "bio_shim"))
sys.path.insert(0, str(REF))

import networkx as nx      # noqa: E402
import numpy as np         # noqa: E402
import pandas as pd        # noqa: E402

from tests import classify_cases as cc      # noqa: E402


def load_reference():
    import pyani.pyani_classify as ref_classify
    spec = importlib.util.spec_from_file_location("ref_subcmd_classify", REF / "pyani" / "scripts" / "subcommands" / "subcmd_classify.py")
    sub = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sub)
    return ref_classify, sub


class ExactFrames:
    """Stands in for the reference module's `pd`: read_json hands back the frame it is given; everything else is pandas."""

    def __getattr__(self, name):
        return getattr(pd, name)

    @staticmethod
    def read_json(frame):
        return frame.copy()


def run_case(name, ref_classify, sub):
    case, par = cc.CASES[name], cc.params(name)
    I, C, labels = cc.build_case(name)
    n = len(I)
    gold = {"case": name, "params": par, "gen": case["gen"], "edits": list(case.get("edits", ())), "n": n, "labels": labels,
            "sha1": cc.sha1_of(I, C), "raises": None, "pandas": pd.__version__, "numpy": np.__version__, "networkx": nx.__version__}
    if n <= 60:
        gold["identity_hex"], gold["coverage_hex"] = I.tobytes().hex(), C.tobytes().hex()
    ids = list(range(n))
    if case.get("json"):
        # real strings: genome ids 1 .. n as the reference's runs store them, and a label dictionary with a gap
        ids = list(range(1, n + 1))
        label_dict = {str(g): f"strain_{g}" for g in ids if g != 3}
        results = types.SimpleNamespace(df_identity=pd.DataFrame(I, index=ids, columns=ids).to_json(),
                                        df_coverage=pd.DataFrame(C, index=ids, columns=ids).to_json())
        gold["json"] = {"df_identity": results.df_identity, "df_coverage": results.df_coverage}
        gold["label_dict"] = label_dict
        gold["labels"] = labels = [f"{label_dict.get(str(g), 'Genome_id')}:{g}" for g in ids]
        saved = None
    else:
        label_dict = {}
        results = types.SimpleNamespace(df_identity=pd.DataFrame(I, index=ids, columns=ids), df_coverage=pd.DataFrame(C, index=ids, columns=ids))
        saved, ref_classify.pd = ref_classify.pd, ExactFrames()
    index = {lab: k for k, lab in enumerate(labels)}
    try:
        t0 = time.perf_counter()
        graph = ref_classify.build_graph_from_results(results, label_dict, par["cov_min"], par["id_min"])
        t1 = time.perf_counter()
        args = Namespace(min_id=par["min_id"], max_id=par["max_id"], resolution=par["resolution"], disable_tqdm=True)
        tuples, parts = [], []
        try:
            for step in sub.trimmed_graph_sequence(graph, args):
                info = step.cliqueinfo
                tuples.append([float(step.interval) if not isinstance(step.interval, int) else step.interval,
                               int(info.n_nodes), int(info.n_subgraphs), bool(info.all_k_complete)])
                if n <= cc.PARTITIONS_UP_TO:      # the yielded graph is the live one: read it before the generator goes on
                    parts.append(sorted(sorted(index[v] for v in comp) for comp in nx.connected_components(step.graph)))
        except IndexError:
            gold["raises"] = "IndexError"
        t2 = time.perf_counter()
    finally:
        if saved is not None:
            ref_classify.pd = saved
    assert gold["raises"] == case.get("raises"), (name, gold["raises"])
    gold["n_edges"] = graph.number_of_edges()
    gold["tuples"] = tuples
    if n <= cc.PARTITIONS_UP_TO:
        gold["partitions"] = parts
    gold["reference_seconds"] = {"graph_build": round(t1 - t0, 3), "sweep": round(t2 - t1, 3)}
    return gold


def main(names):
    ref_classify, sub = load_reference()
    OUT.mkdir(parents=True, exist_ok=True)
    for name in names or list(cc.CASES):
        gold = run_case(name, ref_classify, sub)
        path = OUT / f"{name}.json.gz"
        with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as fo:
            fo.write(json.dumps(gold, sort_keys=True).encode())
        print(f"{name}: n={gold['n']} edges={gold['n_edges']} steps={len(gold['tuples'])} raises={gold['raises']} "
              f"ref {gold['reference_seconds']} -> {path.stat().st_size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
