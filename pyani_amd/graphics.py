"""graphics — the ordering arithmetic of `pyani plot`: the two hierarchical clusterings that order every heatmap, on the GPU.

Every heatmap the reference draws is ordered by a clustering of the result matrix's rows and one of its columns
(pyani/pyani_graphics/mpl/__init__.py:84-136, add_dendrogram: pdist(dfr) / pdist(dfr.T), Euclidean, linkage(method="complete"),
then the `leaves` and `ivl` of scipy's dendrogram; pyani/pyani_graphics/sns/__init__.py:130, sns.clustermap: the same with
method="average"; pyani/scripts/subcommands/subcmd_plot.py:130-139: five matrices per run).  The distances are O(n^3) on one
core there.  Here the device computes the distances and runs the nearest-neighbour chain (pg_cluster_pdist / pg_cluster_linkage /
pg_cluster_linkage_batch); the host does what fixes order: the stable sort of the merge records by height, the union-find
relabelling, the leaf traversal, the labels and the frame handling.  Results EQUAL scipy's: distances and linkage matrices bit for
bit, leaves and labels element for element.

The distribution plots (pyani_graphics/mpl/__init__.py:139-175, pyani_graphics/sns/__init__.py:192-233) are arithmetic too: a histogram
and a Gaussian kernel density estimate over all cells of a matrix.  The device scans, counts and sums (pg_dist_load / pg_dist_hist /
pg_dist_kde); the host fixes bin edges, grid, bandwidth and normalisation (distribution_data, run_distributions, at the end of this file).

Rendering stays out: this module returns what a drawing layer needs (leaf orders, labels in leaf order, linkage matrices, the
re-ordered frame, bars and curves) and needs neither scipy nor matplotlib nor seaborn.  There is no CPU fallback for the device part;
`merges_to_linkage`, `dendrogram_leaves` and `dendrogram_labels` are host-only and need no GPU."""
import io
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Union

import numpy as np
import pandas as pd

from . import _lib
from .engine import Engine, default_engine

METHODS = {"complete": _lib.PG_CLUSTER_COMPLETE, "average": _lib.PG_CLUSTER_AVERAGE}
NONFINITE = "The condensed distance matrix must contain only finite values."      # scipy's text for the same refusal
TOO_FEW = "The number of observations cannot be determined on an empty distance matrix."


class HeatmapOrder(NamedTuple):
    """What heatmap() (pyani_graphics/mpl/__init__.py:295-345) takes from its two dendrograms."""
    row_leaves: List[int]          # rowdend["dendrogram"]["leaves"]: positions in the row-sorted frame
    col_leaves: List[int]
    row_ivl: list                  # rowdend["dendrogram"]["ivl"]
    col_ivl: list
    row_linkage: np.ndarray        # (rows - 1) x 4, scipy's Z
    col_linkage: np.ndarray
    frame: pd.DataFrame            # dfr.sort_index().iloc[row_leaves, col_leaves]: what imshow is given


def _method(method: str) -> int:
    if method not in METHODS:
        raise ValueError(f'method must be "complete" (the mpl backend) or "average" (the seaborn backend), not {method!r}')
    return METHODS[method]


# ---- host: what fixes order -----------------------------------------------------------------------------------------------------
def merges_to_linkage(merges) -> np.ndarray:
    """scipy's Z from the chain's merge records (slot x < slot y, height, size) in merge order: a STABLE sort by height, then every
    row's two slots replaced by the ids of the clusters they currently stand for, smaller first, the new cluster taking id n + row
    (scipy.cluster.hierarchy's nn_chain epilogue).  Finding a root compresses the path behind it; the roots are the same without."""
    merges = np.asarray(merges, dtype=np.float64).reshape(-1, 4)
    n = len(merges) + 1
    Z = merges[np.argsort(merges[:, 2], kind="stable")].copy()
    parent = list(range(2 * n - 1))
    size = [1] * (2 * n - 1)

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    slots = Z[:, :2].astype(np.int64).tolist()
    for row, (x, y) in enumerate(slots):
        rx, ry = find(x), find(y)
        if rx > ry:
            rx, ry = ry, rx
        new = n + row
        parent[rx] = parent[ry] = new
        size[new] = size[rx] + size[ry]
        Z[row, 0], Z[row, 1], Z[row, 3] = rx, ry, size[new]
    return Z


def dendrogram_leaves(Z) -> List[int]:
    """dendrogram(Z)["leaves"] with scipy's defaults: the first column's subtree before the second's.  Iterative: a chain-shaped tree
    of 8192 leaves is as deep as it is long."""
    Z = np.asarray(Z, dtype=np.float64).reshape(-1, 4)
    n = len(Z) + 1
    left, right = Z[:, 0].astype(np.int64).tolist(), Z[:, 1].astype(np.int64).tolist()
    leaves, stack = [], [2 * n - 2]
    while stack:
        node = stack.pop()
        if node < n:
            leaves.append(node)
        else:
            stack.append(right[node - n])
            stack.append(left[node - n])
    return leaves


def _label_list(labels, n: int) -> Optional[list]:
    """add_dendrogram's rule (pyani_graphics/mpl/__init__.py:123-126): an empty mapping means no labels, else the mapping's values
    in its own order, one per observation BY POSITION."""
    if labels is None:
        return None
    labs = list(labels.values()) if isinstance(labels, Mapping) else list(labels)
    if len(labs) == 0:
        return None
    if len(labs) != n:
        raise ValueError("Dimensions of Z and labels must be consistent.")
    return labs


def dendrogram_labels(Z, labels=None) -> list:
    """dendrogram(Z, labels=...)["ivl"]: the labels in leaf order; without labels the leaf numbers as strings."""
    leaves = dendrogram_leaves(Z)
    labs = _label_list(labels, len(leaves))
    return [str(leaf) for leaf in leaves] if labs is None else [labs[leaf] for leaf in leaves]


# ---- device ---------------------------------------------------------------------------------------------------------------------
def _values(x) -> np.ndarray:
    x = np.asarray(x.to_numpy() if isinstance(x, pd.DataFrame) else x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("A 2-dimensional array must be passed.")
    return x


def _refuse_nonfinite(err: _lib.PyaniGpuError):
    if err.code == _lib.PG_E_NONFINITE:
        raise ValueError(NONFINITE) from None
    raise err


def pdist(x, columns: bool = False, engine: Optional[Engine] = None) -> np.ndarray:
    """scipy.spatial.distance.pdist(x), or pdist(x.T) with columns=True: the condensed float64 vector, bit for bit.  ValueError if a
    distance is not finite (where the reference's next call, linkage, raises it)."""
    x = _values(x)
    n = x.shape[1] if columns else x.shape[0]
    if n < 2 or x.size == 0:
        return np.zeros(0, dtype=np.float64)
    try:
        return (engine or default_engine()).cluster_pdist(x, columns=columns)
    except _lib.PyaniGpuError as err:
        _refuse_nonfinite(err)


def linkage(x, method: str = "complete", columns: bool = False, engine: Optional[Engine] = None) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage(pdist(x), method=...) for "complete" and "average", bit for bit: (n - 1) x 4."""
    code = _method(method)
    x = _values(x)
    if (x.shape[1] if columns else x.shape[0]) < 2 or x.size == 0:
        raise ValueError(TOO_FEW)
    try:
        return merges_to_linkage((engine or default_engine()).cluster_linkage(x, method=code, columns=columns))
    except _lib.PyaniGpuError as err:
        _refuse_nonfinite(err)


def _read_frame(dfr) -> pd.DataFrame:
    if isinstance(dfr, str):
        dfr = pd.read_json(io.StringIO(dfr))      # as write_run_plots reads the Run row's strings (subcmd_plot.py:133-137)
    elif not isinstance(dfr, pd.DataFrame):
        dfr = pd.DataFrame(np.asarray(dfr))
    return dfr


def _frame(dfr) -> pd.DataFrame:
    dfr = _read_frame(dfr)
    # rows only, as heatmap() does (pyani_graphics/mpl/__init__.py:309); an index already in order needs no copy of the frame
    return dfr if dfr.index.is_monotonic_increasing else dfr.sort_index()


def _device_matrix(frame: pd.DataFrame):
    """(matrix, transposed): the frame's float64 values as a C-contiguous array without a transposing copy.  pandas keeps a frame of
    one dtype column-major, so to_numpy() is usually the transpose of a contiguous array; the device clusters either orientation of
    a matrix in place, so that array is handed over as it lies and the two orientation flags are swapped."""
    v = frame.to_numpy(dtype=np.float64)
    if v.flags.f_contiguous and not v.flags.c_contiguous:
        return v.T, True
    return np.ascontiguousarray(v), False


def _orders(frames: Sequence[pd.DataFrame], method: str, labels, engine: Optional[Engine]) -> List[HeatmapOrder]:
    code = _method(method)
    mats = [_device_matrix(f) for f in frames]
    for m, _ in mats:
        if min(m.shape) < 2:
            raise ValueError(TOO_FEW)
    for f in frames:      # before any device work: a wrong number of labels is the caller's mistake
        _label_list(labels, f.shape[0]), _label_list(labels, f.shape[1])
    problems = [(m, columns != transposed, code) for m, transposed in mats for columns in (False, True)]      # rows first, then columns
    merges = (engine or default_engine()).cluster_linkage_batch(problems)
    if any(m is None for m in merges):
        raise ValueError(NONFINITE)
    out = []
    for k, f in enumerate(frames):
        zr, zc = merges_to_linkage(merges[2 * k]), merges_to_linkage(merges[2 * k + 1])
        rl, cl = dendrogram_leaves(zr), dendrogram_leaves(zc)
        out.append(HeatmapOrder(rl, cl, dendrogram_labels(zr, labels), dendrogram_labels(zc, labels), zr, zc, f.iloc[rl, cl]))
    return out


def heatmap_order(dfr, method: str = "complete", labels=None, engine: Optional[Engine] = None) -> HeatmapOrder:
    """Everything heatmap() computes before it draws (pyani_graphics/mpl/__init__.py:309-345): the frame sorted by its row index,
    both clusterings, leaves, labels, and the frame as imshow gets it.  method="complete" is the reference's mpl backend,
    method="average" what its seaborn backend's clustermap computes.  labels: the mapping add_dendrogram is given as params.labels
    (its values go to the leaves by position; empty or None: leaf numbers as strings), for both axes as there.
    dfr: a DataFrame, a DataFrame.to_json() string or an array.  ValueError for a non-finite distance or fewer than two rows / columns."""
    return _orders([_frame(dfr)], method, labels, engine)[0]


def run_heatmap_orders(mats: Mapping[str, Union[pd.DataFrame, str]], method: str = "complete", labels=None,
                       engine: Optional[Engine] = None) -> Dict[str, HeatmapOrder]:
    """heatmap_order for all matrices of a run in ONE batched device call (subcmd_plot.py:130-139: ten clusterings).  mats: what
    anim.assemble_run_matrices returns (frames by name) or what anim.run_matrices_to_json returns (the Run row's strings by column
    name), or any other name -> frame / string mapping.  The result is keyed like the input."""
    names = list(mats)
    return dict(zip(names, _orders([_frame(mats[k]) for k in names], method, labels, engine)))


# ---- distribution plots: histogram and Gaussian kernel density estimate ---------------------------------------------------------
# The reference's distribution() (pyani_graphics/mpl/__init__.py:139-175: hist(data, bins=50), gaussian_kde(data) on a 200-point grid;
# pyani_graphics/sns/__init__.py:192-233: histplot and kdeplot with their defaults) computes, per matrix, a histogram and a density over
# all cells.  The device scans, counts and sums (pg_dist_load / pg_dist_hist / pg_dist_kde); the host fixes the floats: bin edges,
# grid, bandwidth and normalisation, with the numpy calls the reference's libraries make, so that they carry the reference's bits.
DIST_METHODS = ("mpl", "seaborn")
DIST_BINS = 50          # hist(data, bins=50)
DIST_GRID = 200         # np.linspace(min, max, 200); seaborn's gridsize
DIST_CUT = 3            # seaborn's cut: the grid reaches 3 bandwidths past the extremes
NOT_FINITE = "array must not contain infs or NaNs"      # scipy's text (gaussian_kde's Cholesky step checks its input)
TOO_FEW_VALUES = "`dataset` input should have multiple elements."      # gaussian_kde's
SINGULAR = ("The data appears to lie in a lower-dimensional subspace of the space in which it is expressed. This has resulted in a "
            "singular data covariance matrix, which cannot be treated using the algorithms implemented in `gaussian_kde`.")


class DistributionData(NamedTuple):
    """What distribution() computes before it draws: the bars of the left panel and the curve of the right one."""
    bin_edges: np.ndarray      # float64[bins + 1]
    counts: np.ndarray         # int64[bins]: np.histogram's
    support: np.ndarray        # float64[200]: the grid of the density
    density: np.ndarray        # float64[200]: gaussian_kde(data)(support)
    bandwidth: float           # the kernel's standard deviation: gaussian_kde's cho_cov[0, 0]


def _dist_method(method: str) -> str:
    if method not in DIST_METHODS:
        raise ValueError(f'method must be "mpl" or "seaborn", not {method!r}')
    return method


def _flat_values(dfr) -> np.ndarray:
    """`dfr.values.flatten()` as float64 (pyani_graphics/mpl/__init__.py:149): row-major, the frame NOT sorted.  The order is part of
    the contract: the bandwidth's sums run in it."""
    if isinstance(dfr, (str, pd.DataFrame)):
        return np.ascontiguousarray(_read_frame(dfr).values.flatten(), dtype=np.float64)
    return np.array(dfr, dtype=np.float64).reshape(-1)


def scott_bandwidth(x: np.ndarray):
    """(bandwidth, sqrt of the kernel covariance) of scipy.stats.gaussian_kde(x) with its default, Scott's factor, by the numpy calls
    scipy makes (_kde.py: weights = ones(n) / n; neff = 1 / sum(weights ** 2); factor = power(neff, -1 / 5); the data covariance
    cov(dataset, rowvar=1, bias=False, aweights=weights); cho_cov = cholesky(covariance) * factor, for one dimension a square root).
    The first is the kernel's standard deviation and enters every exponent; the second is what seaborn spaces its grid by
    (sqrt(covariance), covariance = data covariance * factor ** 2) and may differ from the first in the last bit.
    ValueError for fewer than two values or non-finite ones, LinAlgError for a singular covariance, as gaussian_kde raises them."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    if not n > 1:
        raise ValueError(TOO_FEW_VALUES)
    weights = np.ones(n) / n
    neff = 1 / np.sum(weights ** 2)
    factor = np.power(neff, -1.0 / 5)
    data_cov = np.atleast_2d(np.cov(x[None, :], rowvar=1, bias=False, aweights=weights))
    if not np.isfinite(data_cov[0, 0]):
        raise ValueError(NOT_FINITE)
    if not data_cov[0, 0] > 0.0:
        raise np.linalg.LinAlgError(SINGULAR)
    cho_cov = (np.sqrt(data_cov) * factor).astype(np.float64)
    return float(cho_cov[0, 0]), float(np.sqrt((data_cov * factor ** 2).squeeze()))


def _distribution(x: np.ndarray, method: str, eng) -> DistributionData:
    if x.size == 0:
        raise ValueError("min() arg is an empty sequence")
    lo, hi, n_nan, n_inf = eng.dist_load(x)
    lo, hi = lo + 0.0, hi + 0.0      # a zero extreme is +0.0 whichever of the equal zeros the scan met first
    if n_inf or (n_nan and method == "mpl"):
        # mpl: hist() skips NaN (nanmin / nanmax) and refuses an infinite range; gaussian_kde refuses both.  seaborn drops NaN only.
        raise ValueError(NOT_FINITE)
    used = x[~np.isnan(x)] if n_nan else x
    if used.size == 0:
        raise ValueError(TOO_FEW_VALUES)
    bw, grid_bw = scott_bandwidth(used)
    if method == "mpl":
        edges = np.histogram_bin_edges(np.empty(0), bins=DIST_BINS, range=(lo, hi))      # +-0.5 when lo == hi, then linspace
        support = np.linspace(lo, hi, DIST_GRID)
    else:
        edges = np.histogram_bin_edges(used, "auto", range=(lo, hi))
        support = np.linspace(lo - grid_bw * DIST_CUT, hi + grid_bw * DIST_CUT, DIST_GRID)
    counts = eng.dist_hist(edges)
    sums = eng.dist_kde(support, bw)
    # gaussian_kde.evaluate: every term is weighted 1 / n and scaled by (2 pi) ** (-d / 2) / cho_cov[0, 0]
    norm = np.power(2 * np.pi, -1 / 2) / bw
    return DistributionData(edges, counts, support, sums * norm * (1.0 / used.size), bw)


def distribution_data(dfr, method: str = "mpl", engine: Optional[Engine] = None) -> DistributionData:
    """Everything distribution() computes before it draws, over all cells of the matrix.  method="mpl" is the reference's matplotlib
    backend (pyani_graphics/mpl/__init__.py:149-156): 50 even bins over (min, max), the density on np.linspace(min, max, 200);
    method="seaborn" what histplot and kdeplot compute with their defaults (pyani_graphics/sns/__init__.py:204-213): NaN cells dropped,
    np.histogram_bin_edges(x, "auto"), the grid from min - 3 bw to max + 3 bw.  dfr: a DataFrame, a DataFrame.to_json() string or an
    array.  Raises what the reference raises: ValueError for a NaN or infinite cell (mpl) or fewer than two values,
    numpy.linalg.LinAlgError when all values are equal."""
    _dist_method(method)
    eng = engine or default_engine()
    try:
        return _distribution(_flat_values(dfr), method, eng)
    finally:
        eng.dist_release()


def run_distributions(mats: Mapping[str, Union[pd.DataFrame, str]], method: str = "mpl",
                      engine: Optional[Engine] = None) -> Dict[str, DistributionData]:
    """distribution_data for all matrices of a run (subcmd_plot.py:141-153), each uploaded once.  mats: as for run_heatmap_orders.  The
    result is keyed like the input."""
    _dist_method(method)
    eng = engine or default_engine()
    try:
        return {k: _distribution(_flat_values(mats[k]), method, eng) for k in mats}
    finally:
        eng.dist_release()
