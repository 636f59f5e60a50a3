"""Shared by the classify tests and tools/make_classify_goldens.py: the input generator of the golden cases and an independent
restatement of the clique sweep (pyani/pyani_classify.py:61-165, subcmd_classify.py:122-171) for tests only.

The generator uses integer hashing only (splitmix64 over numpy uint64, values k / 10**6), no numpy random generator, so the test and
the tool build identical bytes on any numpy.  The restatement shares nothing with pyani_amd: edges taken in DESCENDING identity order
into a union-find that keeps per-component node and edge counts (a component is a clique iff edges == s (s - 1) / 2), read off at
the position in the sorted edge list that every step of the reference's pop loop has reached."""
import hashlib

import numpy as np

U = np.uint64


def splitmix64(x):
    x = (np.asarray(x, dtype=U) + U(0x9E3779B97F4A7C15))
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def family_matrices(n, seed, families=8, subfamilies=4, quantum=1, asym=0):
    """(identity, coverage), n x n float64.  Genomes in `families` contiguous blocks, each in `subfamilies` sub-blocks; identity in
    millionths: 970000 / 900000 / 770000 (same sub-family / same family / unrelated) plus a hashed jitter below 25000 / 60000 / 50000,
    rounded down to a multiple of `quantum` (a coarse quantum makes many edges tie); symmetric unless `asym` (then the [i, j], i > j
    cell loses a hashed amount below `asym`).  Coverage: 600000 + jitter below 350000 within a family, 250000 + jitter below 400000
    across, never symmetric.  Diagonals 1."""
    with np.errstate(over="ignore"):
        g = np.arange(n, dtype=np.int64)
        fam = g * families // n
        sub = g * families * subfamilies // n
        i, j = np.meshgrid(g, g, indexing="ij")
        lo, hi = np.minimum(i, j).astype(U), np.maximum(i, j).astype(U)
        h = splitmix64(lo * U(1000003) + hi + (U(seed) << U(40)))
        h2 = splitmix64(i.astype(U) * U(1000003) + j.astype(U) + (U(seed + 1) << U(40)))
        same_fam, same_sub = fam[i] == fam[j], sub[i] == sub[j]
        base = np.where(same_sub, 970000, np.where(same_fam, 900000, 770000)).astype(np.int64)
        span = np.where(same_sub, 25000, np.where(same_fam, 60000, 50000)).astype(U)
        k = base + (h % span).astype(np.int64)
        if asym:
            k = k - np.where(i > j, (h2 % U(asym)).astype(np.int64), 0)
        k = k // quantum * quantum
        cov = np.where(same_fam, 600000, 250000).astype(np.int64) + (h2 % np.where(same_fam, 350000, 400000).astype(U)).astype(np.int64)
    ident = k.astype(np.float64) / 1e6
    cover = cov.astype(np.float64) / 1e6
    np.fill_diagonal(ident, 1.0)
    np.fill_diagonal(cover, 1.0)
    return ident, cover


def _isolate(I, C, g):
    """Genome g keeps no edge under positive floors: its coverage in both directions drops to 0.1."""
    C[g, :] = 0.1
    C[:, g] = 0.1
    C[g, g] = 1.0


# name -> generator arguments, edits and classify parameters.  resolution 1e-3: 12 / 60 genomes trim edge by edge, 200 and up by arange.
DEFAULTS = dict(cov_min=0.5, id_min=0.8, min_id=None, max_id=None, resolution=1e-3)
CASES = {
    "n12_default": dict(gen=dict(n=12, seed=1, families=3, subfamilies=2)),
    "n12_zero_floors": dict(gen=dict(n=12, seed=1, families=3, subfamilies=2), cov_min=0, id_min=0),
    "n12_no_edge": dict(gen=dict(n=12, seed=1, families=3, subfamilies=2), id_min=2.0, raises="IndexError"),
    "n12_no_edge_min_id": dict(gen=dict(n=12, seed=1, families=3, subfamilies=2), id_min=2.0, min_id=0.9),
    "n12_json": dict(gen=dict(n=12, seed=2, families=3, subfamilies=2), json=True, cov_min=0, id_min=0),
    "n60_default": dict(gen=dict(n=60, seed=3, families=4, subfamilies=3)),
    "n60_zero_floors": dict(gen=dict(n=60, seed=3, families=4, subfamilies=3), cov_min=0, id_min=0),
    "n60_coarse": dict(gen=dict(n=60, seed=4, families=4, subfamilies=3, quantum=5000)),
    "n60_min_max": dict(gen=dict(n=60, seed=3, families=4, subfamilies=3), min_id=0.9, max_id=0.98),
    "n60_min_id_zero": dict(gen=dict(n=60, seed=3, families=4, subfamilies=3), min_id=0),
    "n60_nan": dict(gen=dict(n=60, seed=5, families=4, subfamilies=3), edits=["nan"]),
    "n60_last_isolated": dict(gen=dict(n=60, seed=6, families=4, subfamilies=3), edits=["last_isolated"]),
    "n60_middle_isolated": dict(gen=dict(n=60, seed=6, families=4, subfamilies=3), edits=["middle_isolated"]),
    "n60_asymmetric": dict(gen=dict(n=60, seed=7, families=4, subfamilies=3, asym=30000)),
    "n60_identity_one": dict(gen=dict(n=60, seed=8, families=4, subfamilies=3), edits=["ones"]),
    "n200_default": dict(gen=dict(n=200, seed=9, families=5, subfamilies=4)),
    "n200_zero_floors": dict(gen=dict(n=200, seed=9, families=5, subfamilies=4), cov_min=0, id_min=0),
    "n200_min_max": dict(gen=dict(n=200, seed=9, families=5, subfamilies=4), min_id=0.85, max_id=0.99),
    "n200_coarse": dict(gen=dict(n=200, seed=10, families=5, subfamilies=4, quantum=1000), edits=["nan", "ones"]),
    "n400_default": dict(gen=dict(n=400, seed=11, families=5, subfamilies=4)),
    "n1000_default": dict(gen=dict(n=1000, seed=12, families=8, subfamilies=4), resolution=2.5e-4, large=True),
    "n1500_default": dict(gen=dict(n=1500, seed=13, families=12, subfamilies=4), large=True),
}
PARTITIONS_UP_TO = 400      # genomes: the goldens hold every step's partition up to this size


def params(name):
    return {k: CASES[name].get(k, v) for k, v in DEFAULTS.items()}


def build_case(name):
    """(identity, coverage, labels) of a case: the generator's matrices after the case's edits."""
    case = CASES[name]
    I, C = family_matrices(**case["gen"])
    n = len(I)
    for e in case.get("edits", ()):
        if e == "nan":      # NaN in either direction of a pair, in both, in identity and in coverage (Python's min keeps the order)
            I[1, 0] = np.nan; I[2, 5] = np.nan; I[7, 3] = np.nan; I[3, 7] = np.nan
            C[4, 0] = np.nan; C[2, 6] = np.nan; I[n - 1, n - 2] = np.nan; C[n - 3, n - 1] = np.nan
        elif e == "last_isolated":
            _isolate(I, C, n - 1)
        elif e == "middle_isolated":
            _isolate(I, C, n // 2)
        elif e == "ones":      # identity exactly 1.0 off the diagonal, one direction and both
            I[0, 1] = I[1, 0] = 1.0
            I[3, 2] = 1.0
            I[n - 1, n - 2] = I[n - 2, n - 1] = 1.0
    return I, C, [f"Genome_id:{g}" for g in range(n)]


def sha1_of(I, C):
    return hashlib.sha1(np.ascontiguousarray(I).tobytes() + np.ascontiguousarray(C).tobytes()).hexdigest()


# ---- the independent restatement -----------------------------------------------------------------------------------------------
def restate(I, C, cov_min=0.5, id_min=0.8, min_id=None, max_id=None, resolution=1e-4, partitions=False):
    """[(interval, n_nodes, n_subgraphs, all_k_complete)] and, with partitions=True, per step the set of frozensets of node indices."""
    I, C = np.asarray(I, dtype=np.float64), np.asarray(C, dtype=np.float64)
    n = len(I)
    iu, ju = np.triu_indices(n, 1)      # the pair (column i, column j), i < j
    with np.errstate(invalid="ignore"):
        a, b = I[ju, iu], I[iu, ju]
        wi = np.where(b < a, b, a)
        a, b = C[ju, iu], C[iu, ju]
        wc = np.where(b < a, b, a)
        keep = (wi > id_min) & (wc > cov_min)
    iu, ju, wi = iu[keep], ju[keep], wi[keep]
    order = np.argsort(wi, kind="stable")
    iu, ju, ids = iu[order], ju[order], wi[order].tolist()
    in_set = np.zeros(n, dtype=bool)
    in_set[:n - 1] = True
    in_set[iu] = True
    in_set[ju] = True
    n_nodes = int(in_set.sum())
    # the reference's pop loops, as positions in the ascending list: every step sees ids[p:]
    E = len(ids)
    threshold = min_id or ids[0]      # IndexError without edges
    p = 0
    while p < E and ids[p] <= threshold:
        p += 1
    if E - p < 1 / resolution:
        breaks = ids[p:]
    else:
        breaks = np.arange(min_id or ids[p], max_id or 1, resolution)
    seen = []      # (interval, position)
    for t in breaks:
        seen.append((t, p))
        while p < E and ids[p] <= t:
            p += 1
    while p < E and ids[p] <= 1:
        p += 1
    seen.append((1, p))
    # union-find over the edges from the top of the list down; the steps are read off last to first
    parent = list(range(n))
    nodes = [1] * n
    edges = [0] * n
    state = {"components": n_nodes, "incomplete": 0}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def add(x, y):
        rx, ry = find(x), find(y)
        was = [r for r in {rx, ry} if edges[r] != nodes[r] * (nodes[r] - 1) // 2]
        state["incomplete"] -= len(was)
        if rx != ry:
            if nodes[rx] < nodes[ry]:
                rx, ry = ry, rx
            parent[ry] = rx
            nodes[rx] += nodes[ry]
            edges[rx] += edges[ry]
            state["components"] -= 1
        edges[rx] += 1
        if edges[rx] != nodes[rx] * (nodes[rx] - 1) // 2:
            state["incomplete"] += 1

    out, parts = [None] * len(seen), [None] * len(seen)
    at = E
    for k in range(len(seen) - 1, -1, -1):
        interval, pos = seen[k]
        while at > pos:
            at -= 1
            add(int(iu[at]), int(ju[at]))
        out[k] = (interval, n_nodes, state["components"], state["incomplete"] == 0)
        if partitions:
            groups = {}
            for g in np.flatnonzero(in_set).tolist():
                groups.setdefault(find(g), []).append(g)
            parts[k] = {frozenset(v) for v in groups.values()}
    return (out, parts) if partitions else out


def same_float(a, b):
    """Bit-for-bit equality of two numbers taken as float64 (1 and 1.0 are the same interval)."""
    return np.float64(a).tobytes() == np.float64(b).tobytes()
