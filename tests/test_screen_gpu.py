"""GPU (through the C ABI): the screen (pg_screen_matrix, pyani_amd/csrc/pg_screen.hip) against the numpy statement of its definition
(tests/screen_cases.py; checked against brute force and for non-vacuity by tests/test_screen_cpu.py).  Sizes and shared counts are
integers and must equal the statement EXACTLY — whatever the slices, the parts, the order of the ids or the number of devices."""
import numpy as np
import pandas as pd
import pytest

from tests import screen_cases as scr

pytestmark = pytest.mark.gpu


def _load(eng, genomes):
    return [eng.add_genome(s, o) for s, o in genomes]


def _equal(res, want, what):
    sizes, shared = res
    assert sizes.dtype == np.uint32 and shared.dtype == np.uint32, what
    assert (sizes == want[0]).all(), (what, sizes, want[0])
    bad = np.argwhere(shared != want[1])
    assert len(bad) == 0, (what, len(bad), bad[:5], shared[tuple(bad[0])], want[1][tuple(bad[0])])


@pytest.fixture(scope="module")
def family_engine():
    from pyani_amd.engine import Engine
    with Engine(0) as eng:
        yield eng, _load(eng, scr.family())


# ---- family ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,scale", scr.FAMILY_PARAMS)
def test_family_equals_the_statement(family_engine, k, scale):
    eng, ids = family_engine
    _equal(eng.screen_matrix(ids, kmer=k, scale=scale), scr.expected("family", k, scale), ("family", k, scale))
    last = eng.screen_last()
    sizes, shared = scr.expected("family", k, scale)
    assert last["distinct"] == int(sizes.sum()) and last["keys"] >= last["distinct"] and last["slices"] == 1
    assert last["pair_increments"] == int(np.triu(shared.astype(np.int64), 1).sum())
    if (k, scale) == (16, 16):
        assert last["keys"] > last["distinct"]      # the ancestor's repeat: dropped by the grouping, not counted twice


# ---- wide --------------------------------------------------------------------------------------------------------------------------------
def test_wide_groups_of_three_thousand_genomes():
    from pyani_amd.engine import Engine
    k, scale = scr.WIDE_PARAMS
    with Engine(0) as eng:
        ids = _load(eng, scr.wide())
        res = eng.screen_matrix(ids, kmer=k, scale=scale)
        last = eng.screen_last()
    _equal(res, scr.expected("wide", k, scale), "wide")
    assert last["pair_increments"] > 2 ** 25 and last["groups"] >= 9 + 9 + 5


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
def test_edges_orders_and_refusals():
    from pyani_amd import _lib
    from pyani_amd.engine import Engine
    k, scale = scr.EDGES_PARAMS
    genomes = scr.edges()
    want_sizes, want_shared = scr.expected("edges", k, scale)
    with Engine(0) as eng:
        ids = _load(eng, genomes)
        _equal(eng.screen_matrix(ids, kmer=k, scale=scale), (want_sizes, want_shared), "edges")
        for order in (list(range(len(ids)))[::-1], [int(x) for x in np.random.default_rng(5).permutation(len(ids))], [1], [scr.EDGES_N_ONLY], [0, scr.EDGES_TWIN],
                      [scr.EDGES_SHORT, 5], [scr.EDGES_SHORT, scr.EDGES_N_ONLY]):      # descending, shuffled, n = 1, n = 2; the permuted matrix
            o = np.array(order)
            _equal(eng.screen_matrix([ids[i] for i in order], kmer=k, scale=scale), (want_sizes[o], want_shared[np.ix_(o, o)]), ("edges", order))
        s, m = eng.screen_matrix([], kmer=k, scale=scale)
        assert s.shape == (0,) and m.shape == (0, 0)
        refusals = [(dict(ids=[ids[0], ids[1], ids[0]], kmer=k, scale=scale), "twice"), (dict(ids=ids, kmer=7, scale=scale), "8 ... 16"),
                    (dict(ids=ids, kmer=17, scale=scale), "8 ... 16"), (dict(ids=ids, kmer=k, scale=3), "power of two"),
                    (dict(ids=ids, kmer=k, scale=131072), "power of two"), (dict(ids=list(range(8193)), kmer=k, scale=scale), "8192"),
                    (dict(ids=[ids[0], 1000], kmer=k, scale=scale), "out of range"), (dict(ids=ids, kmer=k, scale=scale, part=2, n_parts=2), "n_parts")]
        for kwargs, word in refusals:
            with pytest.raises(_lib.PyaniGpuError) as err:
                eng.screen_matrix(**kwargs)
            assert err.value.code == _lib.PG_E_ARG and word in str(err.value), (kwargs.get("kmer"), word, str(err.value))
            _equal(eng.screen_matrix(ids, kmer=k, scale=scale), (want_sizes, want_shared), ("edges after a refusal", word))      # the engine stays usable


# ---- slices ------------------------------------------------------------------------------------------------------------------------------
def test_slices_and_parts_do_not_change_the_result(family_engine):
    from pyani_amd import _lib
    eng, ids = family_engine
    want = scr.expected("family", 16, 16)
    try:
        one = eng.screen_matrix(ids, kmer=16, scale=16)
        keys = eng.screen_last()["keys"]
        assert eng.screen_last()["slices"] == 1
        eng.screen_set_budget(keys // 3)
        cut = eng.screen_matrix(ids, kmer=16, scale=16)
        last = eng.screen_last()
        assert last["slices"] >= 3 and last["keys"] == keys
        _equal(cut, one, "a third of the keys per slice")
        _equal(cut, want, "a third of the keys per slice, against the statement")
        parts = [eng.screen_matrix(ids, kmer=16, scale=16, part=p, n_parts=3) for p in range(3)]      # (still sliced: a part is cut as the whole is)
        assert all(p[0].sum() > 0 for p in parts)
        _equal((sum(p[0] for p in parts), sum(p[1] for p in parts)), want, "parts 0, 1, 2 of 3 summed")
        eng.screen_set_budget(1)
        with pytest.raises(_lib.PyaniGpuError) as err:
            eng.screen_matrix(ids, kmer=16, scale=16)
        assert err.value.code == _lib.PG_E_NOMEM and "budget" in str(err.value)
        with pytest.raises(_lib.PyaniGpuError) as err:
            eng.screen_set_budget((1 << 30) + 1)
        assert err.value.code == _lib.PG_E_ARG
    finally:
        eng.screen_set_budget(0)
    _equal(eng.screen_matrix(ids, kmer=16, scale=16), want, "the default budget after a refusal")
    assert eng.screen_last()["slices"] == 1


# ---- neighbours --------------------------------------------------------------------------------------------------------------------------
def test_screen_leaves_the_sketch_mode_alone(family_engine):
    eng, ids = family_engine
    q, r = [ids[0], ids[3], ids[5], ids[7]], [ids[4], ids[0], ids[2], ids[0]]
    before = eng.sketch_pairs(q, r, frag_len=1000, scale=16, kmer=16)
    eng.screen_matrix(ids, kmer=16, scale=16)
    eng.screen_matrix(ids, kmer=12, scale=16)
    after = eng.sketch_pairs(q, r, frag_len=1000, scale=16, kmer=16)      # the cached sketches, untouched
    assert before.tobytes() == after.tobytes() and int(before["status"][0]) == 0 and int(before["status"][3]) == 1


# ---- driver ------------------------------------------------------------------------------------------------------------------------------
def _read_tab(path):
    return pd.read_csv(path, sep="\t", index_col=0, float_precision="round_trip")


def test_run_screen_on_the_gpu(synth_ci_dir, tmp_path):
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_screen import run_screen, tab_path
    indir = next(iter(synth_ci_dir.values())).parent
    paths = sorted(synth_ci_dir.values())
    stems = [p.stem for p in paths]
    with Engine(0) as eng:
        run = run_screen(indir, tmp_path, scale=16, write_output=True, engine=eng)
        assert eng.genome_count() == 0      # a store the driver filled itself is cleared
        loaded = eng.add_fasta_batch(paths)
        direct = screen.screen_genomes(eng, [g for g, _, _ in loaded], stems, scale=16)
        again = run_screen(indir, scale=16, engine=eng)
        assert eng.genome_count() == 2 * len(paths)      # ... the caller's is not (the run's own copies stay with it)
    res = run.result
    assert res.labels == stems and list(run.lengths) == stems and run.lengths == {p.stem: t for p, (_, t, _) in zip(paths, loaded)}
    assert (res.kmer, res.scale) == (16, 16) and res.sizes.min() > 1000
    for other in (direct, again.result):
        assert other.labels == res.labels and (other.sizes == res.sizes).all() and (other.shared == res.shared).all()
    ident = res.identity()
    assert list(ident.index) == list(ident.columns) == stems
    off_diagonal = ident.to_numpy()[~np.eye(len(stems), dtype=bool)]
    assert (off_diagonal > 0.95).sum() >= 2 and (off_diagonal < 0.85).sum() >= 2      # the set holds close and distant relatives
    from pyani_amd import synth
    cfg = synth.SETS["CI"]
    _equal((res.sizes, res.shared), scr.statement([synth.genome(cfg["seed"], cfg["n"], g, cfg["L"]) for g in range(cfg["n"])], 16, 16), "the CI set's files")
    frames = {"shared": res.shared_frame(), "containment": res.containment(), "identity": ident}
    for name, frame in frames.items():
        back = _read_tab(tab_path(tmp_path, name))
        assert list(back.index) == list(back.columns) == stems
        assert (back.to_numpy() == frame.to_numpy()).all(), name
    pairs = res.candidate_pairs(0.8)
    assert pairs and all((b, a) in pairs for a, b in pairs) and pairs == sorted(pairs)
    multi = run_screen(indir, scale=16, devices=[0, 0])
    assert multi.result.labels == res.labels and (multi.result.sizes == res.sizes).all() and (multi.result.shared == res.shared).all()
    assert multi.lengths == run.lengths


# ---- estimate ----------------------------------------------------------------------------------------------------------------------------
def test_estimate_within_the_bound_of_the_definition():
    """|identity[ancestor][copy] - fraction of unchanged bases| <= 0.006 for four 200 kb ancestors and their copies at 1 ... 10 %
    substitutions (k = 16, scale 16): about 8 sigma of the binomial error of a containment over ~12 400 sampled k-mers.  The CPU test
    asserts the same bound on the numpy statement, and the integers here must equal the statement's: this can only fail through the kernel."""
    from pyani_amd import screen
    from pyani_amd.engine import Engine
    k, scale = scr.ESTIMATE_PARAMS
    genomes, pairs = scr.estimate()
    with Engine(0) as eng:
        ids = _load(eng, genomes)
        res = screen.screen_genomes(eng, ids, [f"g{i}" for i in range(len(ids))], kmer=k, scale=scale)
    _equal((res.sizes, res.shared), scr.expected("estimate", k, scale), "estimate")
    ident = res.identity().to_numpy()
    errors = [abs(ident[a][c] - same) for a, c, same in pairs]
    print("estimate: worst error", max(errors))
    assert max(errors) <= scr.ESTIMATE_BOUND
    found = set(res.candidate_pairs(0.85))
    assert all((a, c) in found and (c, a) in found for a, c, _ in pairs)
    assert not any((a, b) in found for a, _, _ in pairs for b, _, _ in pairs if a != b)      # two ancestors are never candidates
