"""CPU-only: the screen's definition (pyani_amd/csrc/pg_screen_core.h) as tests/screen_cases.py states it — against brute-force set
intersections, the non-vacuity of every case of tests/test_screen_gpu.py, the estimate's bound on the statement alone — the core
header's triangle decode and bin cut through a stand-alone sanitizer build (tests/screen/tri_check.cpp), the C ABI of the three calls,
and the host arithmetic of pyani_amd/screen.py on hand-made integer matrices."""
import re
import subprocess

import numpy as np
import pytest

from tests import screen_cases as scr
from tests import sketch_k_cases as skc
from tests.conftest import ROOT


# ---- 1. the statement against brute force ------------------------------------------------------------------------------------------------
def _brute_sets(genomes, k, scale):
    """Python sets of sampled canonical k-mers, one window at a time, both strands spelled out."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    out = []
    for seq, off in genomes:
        s = set()
        for r in range(len(off) - 1):
            rec = bytes(seq[int(off[r]):int(off[r + 1])]).decode().upper()
            for p in range(len(rec) - k + 1):
                w = rec[p:p + k]
                if any(c not in code for c in w):
                    continue
                rc = "".join(comp[c] for c in reversed(w))
                fwd = sum(code[c] << (2 * (k - 1 - i)) for i, c in enumerate(w))
                rev = sum(code[c] << (2 * (k - 1 - i)) for i, c in enumerate(rc))
                canon = min(fwd, rev)
                if int(skc.mix32(np.array([canon], dtype=np.uint64))[0]) & (scale - 1) == 0:
                    s.add(canon)
        out.append(s)
    return out


@pytest.mark.parametrize("k,scale", [(16, 4), (9, 2)])
def test_statement_equals_brute_force_set_intersections(k, scale):
    genomes = scr.edges()
    sets = _brute_sets(genomes, k, scale)
    sizes, shared = scr.statement(genomes, k, scale)
    assert sizes.tolist() == [len(s) for s in sets]
    assert shared.tolist() == [[len(a & b) for b in sets] for a in sets]
    assert sizes[0] > 500 and shared[0][1] >= 2      # (the small case is not empty)


# ---- 2. non-vacuity of the GPU cases -----------------------------------------------------------------------------------------------------
def test_family_holds_what_it_is_for():
    genomes = scr.family()
    assert len(genomes) == 8 and all(len(s) == scr.FAMILY_BASES for s, _ in genomes)
    assert sorted({len(o) - 1 for _, o in genomes}) == [1, 2, 3] and all(int(x) % 32 for _, o in genomes for x in o[1:-1])
    for k, scale in scr.FAMILY_PARAMS:
        sizes, shared = scr.expected("family", k, scale)
        assert (shared == shared.T).all() and (np.diag(shared) == sizes).all()
        # the reverse-complemented copy shares as much as the forward copy: all of the ancestor's set
        assert shared[0][scr.FAMILY_RC] == shared[0][scr.FAMILY_FWD] == sizes[0] > 0 and sizes[scr.FAMILY_RC] == sizes[scr.FAMILY_FWD]
    sizes, shared = scr.expected("family", 16, 16)
    occ = scr.genome_occurrences(*genomes[0], 16, 16)
    assert len(occ) > len(np.unique(occ)) == sizes[0]      # some k-mer occurs twice in one genome
    assert shared[0][3] > shared[0][4] > shared[0][5] > 50 and shared[0][scr.FAMILY_UNRELATED] <= 1      # the rates order the family
    assert 0 < shared[0][scr.FAMILY_DIRTY] < sizes[scr.FAMILY_DIRTY]
    sizes8, shared8 = scr.expected("family", 8, 1)
    # k = 8 (32 896 canonical 8-mers): most k-mers are in most genomes, and thousands of groups have size n
    assert sizes8.min() > 25_000 and shared8.min() > 20_000
    held = np.unique(np.concatenate([scr.genome_set(s, o, 8, 1) for s, o in genomes]), return_counts=True)[1]
    assert int((held == len(genomes)).sum()) > 5_000
    assert scr.expected("family", 16, 256)[0].min() > 100


def test_wide_holds_what_it_is_for():
    genomes = scr.wide()
    k, scale = scr.WIDE_PARAMS
    n = len(genomes)
    assert n == scr.WIDE_N == 3000 and n & (n - 1) and all(len(s) == 48 for s, _ in genomes)
    sizes, shared = scr.expected("wide", k, scale)
    sets = [scr.genome_set(s, o, k, scale) for s, o in genomes]
    everywhere = functools_reduce_intersect(sets)
    assert len(everywhere) == 9                                   # a group of size 3000, nine times
    groups = np.unique(np.concatenate(sets), return_counts=True)[1]
    assert groups.max() == n and int((groups * (groups - 1) // 2).sum()) > 2 ** 25      # P
    assert shared.min() == 9 and shared[0][n - 1] == shared[n - 1][0] == 18 and shared[0][1] == 9      # the corner cells
    # motif 3: forward against reverse-complemented 9 + 5; two of one kind share the 15 k-mers across the two motifs as well (a few more
    # where their four random bases agree)
    assert 14 <= shared[4][1] <= 18 and 29 <= shared[4][8] <= 33 and 29 <= shared[1][3] <= 33 and shared[4][2] == 9


def functools_reduce_intersect(sets):
    out = sets[0]
    for s in sets[1:]:
        out = np.intersect1d(out, s)
    return out


def test_edges_hold_what_they_are_for():
    k, scale = scr.EDGES_PARAMS
    sizes, shared = scr.expected("edges", k, scale)
    assert sizes[scr.EDGES_SHORT] == 0 and sizes[scr.EDGES_N_ONLY] == 0
    assert not shared[scr.EDGES_SHORT].any() and not shared[:, scr.EDGES_N_ONLY].any()
    assert shared[0][scr.EDGES_TWIN] == sizes[0] == sizes[scr.EDGES_TWIN] > 500
    assert 2 <= shared[0][1] < sizes[0]


def test_estimate_bound_holds_on_the_statement():
    """|identity[ancestor][copy] - fraction of unchanged bases| <= 0.006 on the numpy statement alone: the GPU test asserts the same
    bound on the same pairs, so it can only fail through the kernel."""
    k, scale = scr.ESTIMATE_PARAMS
    genomes, pairs = scr.estimate()
    sizes, shared = scr.expected("estimate", k, scale)
    ident = scr.identity_of(sizes, shared, k)
    assert len(pairs) == 20 and 11_000 < sizes.min() and sizes.max() < 14_000
    worst = max(abs(ident[a][c] - same) for a, c, same in pairs)
    print("estimate on the statement: worst error", worst)
    assert worst <= scr.ESTIMATE_BOUND
    other = [ident[a][b] for a, _, _ in pairs for b, _, _ in pairs if a != b]
    assert max(other) < 0.7       # two ancestors share a chance k-mer or two at most: far below any threshold a screen would use


# ---- 3. the core header on the host, under sanitizers --------------------------------------------------------------------------------------
def test_core_header_decode_and_bins_under_sanitizers(tmp_path):
    src = ROOT / "tests" / "screen" / "tri_check.cpp"
    exe = tmp_path / "tri_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "WRONG" not in out.stdout and out.stdout.count("ok ") == 4, out.stdout + out.stderr
    assert "ok rows 67100672" in out.stdout      # two items of every row, m = 2 ... 8192


# ---- 4. the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_library_agree_on_the_screen_calls():
    from pyani_amd import _lib, build
    build.build_gpu()
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    for sym, arity in (("pg_screen_matrix", 9), ("pg_screen_set_budget", 2), ("pg_screen_last", 3)):
        m = re.search(rf"\bint {sym}\s*\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[sym][1]) and hasattr(lib, sym), sym
    assert re.search(r"#define PG_K__END 23\b", text) and re.search(r"#define PG_K__COUNT 20\b", text)      # no new profiling slot
    core = (ROOT / "pyani_amd" / "csrc" / "pg_screen_core.h").read_text()
    assert "screen_tri_decode" in core and "pg_sketch_core.h" in core


# ---- 5. the host arithmetic ------------------------------------------------------------------------------------------------------------------
def _result(sizes, shared, k=16):
    from pyani_amd.screen import ScreenResult
    n = len(sizes)
    return ScreenResult([f"g{i}" for i in range(n)], k, 16, np.array(sizes, dtype=np.uint32), np.array(shared, dtype=np.uint32))


def test_identity_containment_and_nan_rules():
    r = _result([100, 50, 0, 80], [[100, 25, 0, 1], [25, 50, 0, 0], [0, 0, 0, 0], [1, 0, 0, 80]])
    c = r.containment()
    assert list(c.index) == list(c.columns) == ["g0", "g1", "g2", "g3"]
    assert c.loc["g0", "g1"] == 0.25 and c.loc["g1", "g0"] == 0.5 and c.loc["g0", "g0"] == 1.0      # the query on the rows
    assert c.loc["g2"].isna().all() and not c.drop(index="g2").isna().any().any()                   # NaN where size[a] == 0, nowhere else
    j = r.jaccard()
    assert j.loc["g0", "g1"] == j.loc["g1", "g0"] == 25 / 125 and np.isnan(j.loc["g2", "g2"]) and j.loc["g2", "g0"] == 0.0
    i = r.identity()
    assert i.loc["g0", "g1"] == pytest.approx(0.25 ** (1 / 16), rel=1e-15) and i.loc["g1", "g0"] == pytest.approx(0.5 ** (1 / 16), rel=1e-15) and i.loc["g3", "g3"] == 1.0
    assert i.loc["g0", "g3"] == 0.0 and i.loc["g3", "g0"] == 0.0      # one shared k-mer: below the floor
    assert (i.loc["g2"] == 0.0).all() and (i["g2"] == 0.0).all()
    assert r.identity(min_shared=1).loc["g0", "g3"] == pytest.approx(0.01 ** (1 / 16), rel=1e-15)
    assert r.identity(min_shared=26).loc["g0", "g1"] == 0.0
    assert _result([100, 50], [[100, 25], [25, 50]], k=8).identity().loc["g0", "g1"] == pytest.approx(0.25 ** (1 / 8), rel=1e-15)


def test_candidate_pairs_rules():
    # g0-g1 related both ways; g0-g2: high from g2's side only (g2 is small and contained in g0); g3 unrelated; g4 empty
    r = _result([1000, 900, 100, 500, 0],
                [[1000, 600, 90, 1, 0], [600, 900, 3, 0, 0], [90, 3, 100, 0, 0], [1, 0, 0, 500, 0], [0, 0, 0, 0, 0]])
    ident = r.identity().to_numpy()
    assert ident[2][0] > 0.99 > 0.9 > ident[0][2] > 0.8
    assert r.candidate_pairs(0.99) == [(0, 2), (2, 0)]                                  # the larger of the two directions decides, both are listed
    assert r.candidate_pairs(0.95) == [(0, 1), (0, 2), (1, 0), (2, 0)]                  # row-major, never (a, a)
    assert r.candidate_pairs(0.5) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]   # g3 shares one k-mer, g4 nothing: never candidates
    assert r.candidate_pairs(0.5, min_shared=1) == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (2, 0), (2, 1), (3, 0)]
    assert r.candidate_pairs(0.5, min_shared=4) == [(0, 1), (0, 2), (1, 0), (2, 0)]
    assert r.candidate_pairs(1.01) == []


def test_parameter_checks_make_no_library_call():
    from pyani_amd import screen
    assert screen.check_params(16, 256) == (16, 256) and screen.check_params(8, 1) == (8, 1) and screen.check_params(12, 65536) == (12, 65536)
    for k, s in ((7, 16), (17, 16), (16, 3), (16, 0), (16, 131072), (12.5, 16)):
        with pytest.raises(ValueError):
            screen.check_params(k, s)
    with pytest.raises(ValueError):
        screen.screen_genomes(None, [0, 1], ["a", "a"])
    with pytest.raises(ValueError):
        screen.screen_genomes(None, [0, 1], ["a"])
    from pyani_amd.subcmd_screen import run_screen
    with pytest.raises(ValueError):
        run_screen("nowhere", write_output=True)
