"""Shared by the heatmap tests and tools/make_heatmap_goldens.py: the input generator of the golden cases, the golden file format,
and an independent numpy restatement of the clustering that orders the reference's heatmaps (scipy's pdist, Euclidean; scipy's
nearest-neighbour-chain linkage for "complete" and "average"; its relabelling; its leaf order) for tests only.

Inputs are made by integer hashing (tests/classify_cases.py: splitmix64, family_matrices), so the tests and the tool build identical
bytes on any numpy and only RESULTS are stored.  The restatement shares nothing with pyani_amd: distances accumulate in k order on
64 K-cell tiles with one numpy call per operation (every operation rounded on its own), the chain runs on a square matrix whose
dead rows and columns hold +inf, so that numpy's argmin (first occurrence) is "the lowest live index attaining the minimum"."""
import hashlib
import io
import json
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import pandas as pd

from tests.classify_cases import U, family_matrices, splitmix64

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "heatmap"
METHODS = ("complete", "average")
ORIENTATIONS = ("row", "col")
FULL_DISTANCES_UP_TO = 300      # observations: condensed distances stored in full up to here, as a SHA-1 of their bytes beyond
RESTATE_DISTANCES_UP_TO = 1100  # observations: the CPU test restates distances of every case up to here in full detail (seconds)

# name -> how the frame(s) are made.  kind: "ident" (family_matrices identity), "rect", "equal", "run" (five matrices of a run).
CASES = {
    "n2": dict(kind="ident", gen=dict(n=2, seed=31, families=1, subfamilies=1)),
    "n3": dict(kind="ident", gen=dict(n=3, seed=32, families=1, subfamilies=1)),
    "n12": dict(kind="ident", gen=dict(n=12, seed=33, families=3, subfamilies=2)),
    "n63": dict(kind="ident", gen=dict(n=63, seed=34, families=4, subfamilies=3)),
    "n64": dict(kind="ident", gen=dict(n=64, seed=35, families=4, subfamilies=3)),
    "n65": dict(kind="ident", gen=dict(n=65, seed=36, families=4, subfamilies=3)),
    "n128": dict(kind="ident", gen=dict(n=128, seed=37, families=5, subfamilies=3)),
    "n129": dict(kind="ident", gen=dict(n=129, seed=38, families=5, subfamilies=3)),
    "n250_asymmetric": dict(kind="ident", gen=dict(n=250, seed=39, families=6, subfamilies=4, asym=30000)),
    "n40_duplicates": dict(kind="ident", gen=dict(n=40, seed=40, families=3, subfamilies=2), edits=["duplicates"]),
    "n60_two_decimals": dict(kind="ident", gen=dict(n=60, seed=41, families=4, subfamilies=3), edits=["round2"]),
    "n20_all_equal": dict(kind="equal", n=20),
    "rect_40x70": dict(kind="rect", rows=40, cols=70, seed=42),
    "n30_scrambled_index": dict(kind="ident", gen=dict(n=30, seed=43, families=3, subfamilies=2, asym=20000), edits=["scramble"]),
    "n12_labels": dict(kind="ident", gen=dict(n=12, seed=44, families=3, subfamilies=2), labels=True),
    "n12_run_json": dict(kind="run", gen=dict(n=12, seed=45, families=3, subfamilies=2, asym=15000)),
    "n1000": dict(kind="ident", gen=dict(n=1000, seed=46, families=8, subfamilies=4, asym=30000)),
    "n2000": dict(kind="ident", gen=dict(n=2000, seed=47, families=10, subfamilies=4, asym=30000)),
    "n3072": dict(kind="ident", gen=dict(n=3072, seed=48, families=12, subfamilies=4, asym=30000)),
    "n12_nan_cell": dict(kind="ident", gen=dict(n=12, seed=33, families=3, subfamilies=2), edits=["nan"], raises="ValueError"),
    "n1_single": dict(kind="ident", gen=dict(n=1, seed=49, families=1, subfamilies=1), raises="ValueError"),
}


def build_case(name):
    """(frames, labels): frames is {matrix name: DataFrame or DataFrame.to_json() string}; labels the mapping handed to the drawing
    layer as params.labels ({} for none)."""
    case = CASES[name]
    labels = {}
    if case["kind"] == "equal":
        frames = {"m": pd.DataFrame(np.full((case["n"], case["n"]), 0.9))}
    elif case["kind"] == "rect":
        r, c = case["rows"], case["cols"]
        with np.errstate(over="ignore"):
            h = splitmix64(np.arange(r * c, dtype=U) + (U(case["seed"]) << U(40))).reshape(r, c)
        frames = {"m": pd.DataFrame((h % U(250000)).astype(np.float64) / 1e6 + 0.75)}
    elif case["kind"] == "run":
        # the five matrices of a run as the Run row stores them (integer genome ids from 1, values up to 10^6 in aln_lengths)
        from pyani_amd.anim import run_matrices_to_json
        I, C = family_matrices(**case["gen"])
        n = len(I)
        ids = list(range(1, n + 1))
        with np.errstate(over="ignore"):
            length = 800000.0 + (splitmix64(np.arange(n, dtype=U) + U(977)) % U(200000)).astype(np.float64)
        aln = np.floor(C * length[:, None])
        sim = np.floor((1.0 - I) * aln)
        mats = {"identity": I, "coverage": C, "aln_lengths": aln, "sim_errors": sim, "hadamard": I * C}
        strings = run_matrices_to_json({k: pd.DataFrame(v, index=ids, columns=ids) for k, v in mats.items()})
        return strings, labels
    else:
        I, _ = family_matrices(**case["gen"])
        n = len(I)
        index = columns = list(range(n))
        for e in case.get("edits", ()):
            if e == "duplicates":      # genomes 5, 6 copy genome 4 and genome 30 copies genome 29: zero distances, tied heights
                for dst, src in ((5, 4), (6, 4), (30, 29)):
                    I[dst, :] = I[src, :]
                    I[:, dst] = I[:, src]
            elif e == "round2":
                I = np.round(I, 2)
            elif e == "nan":
                I[3, 7] = np.nan
            elif e == "scramble":      # integer labels, rows in scrambled order: heatmap() sorts the rows back, not the columns
                with np.errstate(over="ignore"):
                    perm = np.argsort(splitmix64(np.arange(n, dtype=U) + U(4242)), kind="stable")
                I = I[perm]
                index = [int(p) + 100 for p in perm]
                columns = [c + 100 for c in columns]
        if case.get("labels"):
            labels = {g: f"strain {chr(65 + g)}" for g in range(n)}
        frames = {"m": pd.DataFrame(I, index=index, columns=columns)}
    return frames, labels


def as_frame(f):
    """A case's frame the way the reference receives it (write_run_plots reads the stored strings with pd.read_json)."""
    return pd.read_json(io.StringIO(f)) if isinstance(f, str) else f


def observations(frame, orientation):
    """The matrix whose ROWS are the observations of a clustering of the row-sorted frame."""
    x = frame.sort_index().to_numpy(dtype=np.float64)
    return np.ascontiguousarray(x if orientation == "row" else x.T)


def sha1(a):
    return hashlib.sha1(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- golden files: one .npz per case -------------------------------------------------------------------------------------------
def pack_z(Z):
    """(n - 1) x 4 float64 as exact int32 columns (two ids, size) plus the float64 heights: the heights' bits are kept."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4)
    ints = Z[:, [0, 1, 3]].astype(np.int32)
    assert (ints == Z[:, [0, 1, 3]]).all()
    return ints, np.ascontiguousarray(Z[:, 2])


def unpack_z(ints, heights):
    Z = np.empty((len(heights), 4), dtype=np.float64)
    Z[:, [0, 1, 3]] = ints
    Z[:, 2] = heights
    return Z


def load_gold(name):
    """(meta, arrays): meta is the JSON record, arrays the npz members (keys "<matrix>|<row/col>|..." as the tool writes them)."""
    with np.load(GOLDEN_DIR / f"{name}.npz", allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files if k != "meta"}
        meta = json.loads(str(z["meta"]))
    return meta, arrays


def gold_z(arrays, key, method, what="Z"):
    return unpack_z(arrays[f"{key}|{method}|{what}i"], arrays[f"{key}|{method}|{what}h"])


# ---- the independent restatement -----------------------------------------------------------------------------------------------
def restate_pdist(X, tile=256, threads=None):
    """Condensed Euclidean distances between the rows of X: per pair s = 0; for k ascending: d = u[k] - v[k]; s = s + d * d; sqrt(s)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, m = X.shape
    XT = np.ascontiguousarray(X.T)      # XT[k] is contiguous
    S = np.zeros((n, n), dtype=np.float64)
    tiles = [(i0, j0) for i0 in range(0, n, tile) for j0 in range(i0, n, tile)]

    def run(t):
        i0, j0 = t
        a, b = XT[:, i0:i0 + tile], XT[:, j0:j0 + tile]
        s = np.zeros((a.shape[1], b.shape[1]), dtype=np.float64)
        d = np.empty_like(s)
        for k in range(m):
            np.subtract(a[k][:, None], b[k][None, :], out=d)
            np.multiply(d, d, out=d)
            np.add(s, d, out=s)
        S[i0:i0 + tile, j0:j0 + tile] = np.sqrt(s)

    threads = threads or min(8, os.cpu_count() or 1)
    if threads > 1 and len(tiles) > 1:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(run, tiles))
    else:
        for t in tiles:
            run(t)
    return S[np.triu_indices(n, 1)]


def restate_chain(dists, n, method):
    """The n - 1 merge records (lower slot, higher slot, height, size) of the nearest-neighbour chain, in merge order."""
    D = np.full((n, n), np.inf, dtype=np.float64)
    iu = np.triu_indices(n, 1)
    D[iu] = dists
    D.T[iu] = dists
    size = [1] * n
    chain, merges = [], np.zeros((n - 1, 4), dtype=np.float64)
    lowest = 0
    for step in range(n - 1):
        if not chain:
            while size[lowest] == 0:
                lowest += 1
            chain.append(lowest)
        while True:
            x = chain[-1]
            row = D[x]
            i = int(np.argmin(row))      # first occurrence: the lowest live index attaining the minimum (dead and own cells are +inf)
            if len(chain) > 1:
                y, cur = chain[-2], D[x, chain[-2]]
                if row[i] < cur:
                    y, cur = i, row[i]
                if y == chain[-2]:
                    break
            else:
                y, cur = i, row[i]
            chain.append(y)
        chain.pop()
        chain.pop()
        lo, hi = (x, y) if x < y else (y, x)
        nlo, nhi = size[lo], size[hi]
        merges[step] = (lo, hi, cur, nlo + nhi)
        if method == "complete":
            new = np.maximum(D[lo], D[hi])
        elif method == "average":
            new = (np.float64(nlo) * D[lo] + np.float64(nhi) * D[hi]) / np.float64(nlo + nhi)
        else:
            raise ValueError(method)
        size[lo], size[hi] = 0, nlo + nhi
        D[hi, :] = new
        D[:, hi] = new
        D[hi, hi] = np.inf
        D[lo, :] = np.inf
        D[:, lo] = np.inf
    return merges


def restate_label(merges):
    """scipy's Z: the records sorted by height (stable), slots replaced by current cluster ids (smaller first), new id n + row.
    A plain union-find without path compression."""
    n = len(merges) + 1
    Z = merges[np.argsort(merges[:, 2], kind="stable")].copy()
    parent = list(range(2 * n - 1))
    members = [1] * (2 * n - 1)
    for row in range(n - 1):
        roots = []
        for v in (int(Z[row, 0]), int(Z[row, 1])):
            while parent[v] != v:
                v = parent[v]
            roots.append(v)
        a, b = min(roots), max(roots)
        parent[a] = parent[b] = n + row
        members[n + row] = members[a] + members[b]
        Z[row, 0], Z[row, 1], Z[row, 3] = a, b, members[n + row]
    return Z


def restate_leaves(Z):
    n = len(Z) + 1
    out, stack = [], [2 * n - 2]
    while stack:
        v = stack.pop()
        if v < n:
            out.append(v)
        else:
            stack += [int(Z[v - n, 1]), int(Z[v - n, 0])]
    return out


def restate_ivl(leaves, labels):
    labs = list(labels.values())
    return [str(v) for v in leaves] if not labs else [labs[v] for v in leaves]
