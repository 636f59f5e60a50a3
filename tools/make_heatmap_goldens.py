#!/usr/bin/env python3
"""Generate tests/golden/heatmap/*.npz for the cases of tests/heatmap_cases.py.

Runs only where the reference tree exists (a checkout beside this repository, or $PYANI_REFERENCE) together with scipy and
matplotlib.  method="complete": the reference's OWN pyani_graphics.mpl.add_dendrogram is run (Agg backend) on the row-sorted frame,
as heatmap() calls it, and its dendrogram's `leaves` and `ivl` are stored; its module imports without seaborn once
`pyani.pyani_graphics` is entered in sys.modules as an empty package.  method="average": seaborn is not available, so that leg makes
the scipy calls seaborn's clustermap makes with its defaults (pdist Euclidean, linkage(method="average"), dendrogram) — scipy's
answer, not the reference's own run; the metadata says so.  Z and the distances are scipy's, float bits kept.

The test-only restatement (tests/heatmap_cases.py) is run on every case and must equal scipy everywhere — distances, Z for both
methods, leaves — or the tool stops: a difference means the restatement is wrong.  Its merge records (chain order) are stored too,
for the test of the product's host pieces.  DATA only — no reference source text is written anywhere.

Usage: python tools/make_heatmap_goldens.py [case ...]"""
import json
import os
import sys
import types
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("PYANI_REFERENCE", ROOT.parent / "reference"))
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools" / "bio_shim"))
sys.path.insert(0, str(REF))

import matplotlib      # noqa: E402
matplotlib.use("Agg")
import matplotlib.pyplot as plt      # noqa: E402
from matplotlib import gridspec      # noqa: E402
import numpy as np                   # noqa: E402
import pandas as pd                  # noqa: E402
import scipy                         # noqa: E402
import scipy.cluster.hierarchy as sch      # noqa: E402
from scipy.spatial import distance   # noqa: E402

from tests import heatmap_cases as hc      # noqa: E402


def load_reference():
    pkg = types.ModuleType("pyani.pyani_graphics")
    pkg.__path__ = [str(REF / "pyani" / "pyani_graphics")]
    sys.modules["pyani.pyani_graphics"] = pkg
    import pyani.pyani_graphics.mpl as ref_mpl
    return ref_mpl


def reference_dendrogram(ref_mpl, frame, labels, orientation):
    fig = plt.figure(figsize=(4, 4))
    try:
        gs = gridspec.GridSpec(2, 2, wspace=0.0, hspace=0.0, width_ratios=[0.3, 1], height_ratios=[0.3, 1])
        params = types.SimpleNamespace(labels=labels)
        return ref_mpl.add_dendrogram(frame, fig, params, gs, orientation=orientation)["dendrogram"]
    finally:
        plt.close(fig)


def scipy_dendrogram(Z, labels):
    return sch.dendrogram(Z, no_plot=True, labels=list(labels.values()) or None, get_leaves=True)


def run_case(name, ref_mpl):
    case = hc.CASES[name]
    frames, labels = hc.build_case(name)
    meta = {"case": name, "raises": None, "matrices": {}, "scipy": scipy.__version__, "numpy": np.__version__, "pandas": pd.__version__,
            "matplotlib": matplotlib.__version__,
            "provenance": {"complete": "leaves and ivl from the reference's own pyani_graphics.mpl.add_dendrogram; Z and distances from the "
                                       "scipy calls it makes",
                           "average": "scipy's answer to the calls seaborn's clustermap makes (pdist Euclidean, linkage average, "
                                      "dendrogram); seaborn was not available, so this is not the reference's own run"}}
    arrays = {}
    for mat, f in frames.items():
        frame = hc.as_frame(f).sort_index()      # heatmap() sorts before it clusters
        meta["matrices"][mat] = {}
        for o in hc.ORIENTATIONS:
            key = f"{mat}|{o}"
            try:
                dend = reference_dendrogram(ref_mpl, frame, labels, o)
            except ValueError as err:
                meta["raises"] = "ValueError"
                meta["message"] = str(err)
                continue
            X = hc.observations(frame, o)
            n = len(X)
            dists = distance.pdist(X)
            assert hc.same_bits(dists, distance.pdist(frame if o == "row" else frame.T))
            mine = hc.restate_pdist(X)
            if not hc.same_bits(mine, dists):
                raise SystemExit(f"{name} {key}: the restated distances differ from scipy's")
            rec = {"n": n, "m": X.shape[1], "dist_sha1": hc.sha1(dists)}
            if n <= hc.FULL_DISTANCES_UP_TO:
                arrays[f"{key}|dist"] = dists
            for method in hc.METHODS:
                Z = sch.linkage(dists, method=method)
                merges = hc.restate_chain(dists, n, method)
                if not hc.same_bits(hc.restate_label(merges), Z):
                    raise SystemExit(f"{name} {key} {method}: the restated linkage differs from scipy's")
                d = dend if method == "complete" else scipy_dendrogram(Z, labels)
                if method == "complete":
                    again = scipy_dendrogram(Z, labels)
                    assert again["leaves"] == d["leaves"] and again["ivl"] == d["ivl"]
                if hc.restate_leaves(Z) != d["leaves"] or hc.restate_ivl(d["leaves"], labels) != d["ivl"]:
                    raise SystemExit(f"{name} {key} {method}: the restated leaves differ from scipy's")
                arrays[f"{key}|{method}|Zi"], arrays[f"{key}|{method}|Zh"] = hc.pack_z(Z)
                arrays[f"{key}|{method}|Mi"], arrays[f"{key}|{method}|Mh"] = hc.pack_z(merges)
                arrays[f"{key}|{method}|leaves"] = np.asarray(d["leaves"], dtype=np.int32)
                rec[method] = {"ivl": d["ivl"]}
            meta["matrices"][mat][o] = rec
    assert meta["raises"] == case.get("raises"), (name, meta["raises"])
    if meta["raises"]:
        arrays, meta["matrices"] = {}, {}
    return meta, arrays


def main(names):
    ref_mpl = load_reference()
    hc.GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
    for name in names or list(hc.CASES):
        meta, arrays = run_case(name, ref_mpl)
        path = hc.GOLDEN_DIR / f"{name}.npz"
        np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
        print(f"{name}: raises={meta['raises']} arrays={len(arrays)} -> {path.stat().st_size} bytes", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
