"""GPU (through the C ABI): the MAPPED sketch mode (mapping = "window": pg_sketch_pairs_mapped, pg_sketch_pair_fragments,
pyani_amd/csrc/pg_sketch.hip) against the numpy statement of its definition (tests/sketch_map_cases.py; checked for non-vacuity by
tests/test_sketch_map_cpu.py) — matches, fragments and status equal, the ANI estimate BIT-equal — the per-fragment records rule by
rule, the mode beside the unchanged "anywhere" mode on one engine, the capacity limit, one call of many pairs, the run_fastani driver,
and both mappings priced against the exact engine at k = 16, 14, 12."""
import ctypes
import json
import os
from pathlib import Path

import numpy as np
import pytest

from tests import sketch_cases as sc
from tests import sketch_k_cases as skc
from tests import sketch_map_cases as smc

pytestmark = pytest.mark.gpu


def _load(eng, case):
    return [eng.add_genome(s, o) for s, o in case.genomes]


def _run(eng, ids, pairs, name, mapping="window", **over):
    _, k, frag_len, scale, minfrac = smc.SETS[name]
    kw = dict(frag_len=frag_len, scale=scale, min_fraction=minfrac, kmer=k)
    kw.update(over)
    return eng.sketch_pairs([ids[q] for q, _ in pairs], [ids[r] for _, r in pairs], mapping=mapping, **kw)


def _results(name, pairs=None):
    return [a[0] for a in smc.answers(name, pairs)]


# ---- 3. the GPU equals the definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["family_k8", "family_k12", "family_k16", "rules", "records_k8", "records_k15", "edges", "repeats", "wide"])
def test_mapped_pairs_equal_the_definition_bit_for_bit(name):
    from pyani_amd.engine import Engine
    case = smc.SETS[name][0]()
    want = _results(name)
    with Engine(0) as eng:
        ids = _load(eng, case)
        res = _run(eng, ids, case.pairs, name)
        again = _run(eng, ids, case.pairs[::-1], name)      # the cached index and grouped sketches, another order
    sc.assert_records_equal(res, want, name)
    assert again[::-1].tobytes() == res.tobytes()


# ---- 4. the detail call -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rules", "repeats"])
def test_pair_fragments_equal_the_definition_rule_by_rule(name):
    from pyani_amd.engine import Engine
    case = smc.SETS[name][0]()
    _, k, frag_len, scale, minfrac = smc.SETS[name]
    with Engine(0) as eng:
        ids = _load(eng, case)
        pair_call = _run(eng, ids, case.pairs, name)
        for (q, r), whole in zip(case.pairs, pair_call):
            _, want, _ = smc.answer(name, q, r)
            got = eng.sketch_pair_fragments(ids[q], ids[r], frag_len=frag_len, scale=scale, kmer=k)
            assert len(got) == len(want) == int(whole["fragments"])
            have = [(int(x["window"]), int(x["bin"]), int(x["hits"]), int(x["n"]), int(x["kept"])) for x in got]
            assert have == [(w, b, h, n, kept) for w, b, h, n, _, kept in want], (name, q, r)
            assert [float(x["identity"]).hex() for x in got] == [float(w[4]).hex() for w in want], (name, q, r)
            assert not got["reserved"].any()
            total, matches = 0.0, 0      # the survivors summed again on the host, in fragment order
            for x in got:
                if x["kept"]:
                    total = total + float(x["identity"]); matches += 1
            assert matches == int(whole["matches"])
            enough = matches > 0 and float(matches) >= minfrac * len(got)
            assert float(whole["ani"]).hex() == float(total / matches if enough else 0.0).hex()
        # cap smaller than the count: PG_OK, the first `cap` records written, the count returned
        q, r = case.pairs[0]
        full = eng.sketch_pair_fragments(ids[q], ids[r], frag_len=frag_len, scale=scale, kmer=k)
        part = np.zeros(3, dtype=Engine.SKETCH_FRAGMENT_DTYPE)
        part["hits"][2] = 12345      # beyond the cap: stays as it is
        n = ctypes.c_uint64(0)
        eng._check(eng.lib.pg_sketch_pair_fragments(eng._h, ids[q], ids[r], k, frag_len, scale, part.ctypes.data, 2, ctypes.byref(n)))
        assert n.value == len(full) > 3 and part[:2].tobytes() == full[:2].tobytes() and int(part["hits"][2]) == 12345
        eng._check(eng.lib.pg_sketch_pair_fragments(eng._h, ids[q], ids[r], k, frag_len, scale, None, 0, ctypes.byref(n)))
        assert n.value == len(full)
        build_ms, map_ms = eng.sketch_map_last_ms()
        assert build_ms == 0.0 and map_ms > 0.0      # everything was cached; the kernel ran


# ---- 5. the mode leaves the other one alone ---------------------------------------------------------------------------------------------------
def test_mapped_and_anywhere_on_one_engine():
    from pyani_amd.engine import Engine
    case, other = smc.family(12), smc.family(16)
    pairs = case.pairs
    with Engine(0) as eng:      # a fresh engine that never maps
        ids = _load(eng, case)
        fresh_1000 = _run(eng, ids, pairs, "family_k12", mapping="anywhere")
        fresh_500 = _run(eng, ids, pairs, "family_k12_L500", mapping="anywhere")
    with Engine(0) as eng:
        ids = _load(eng, case)
        q = np.ascontiguousarray([ids[a] for a, _ in pairs], dtype=np.int32)
        r = np.ascontiguousarray([ids[b] for _, b in pairs], dtype=np.int32)

        def old_entry():
            out = np.zeros(len(q), dtype=Engine.SKETCH_DTYPE)
            eng._check(eng.lib.pg_sketch_pairs(eng._h, q.ctypes.data, r.ctypes.data, len(q), 3000, 16, 0.2, out.ctypes.data))
            return out
        old_before = old_entry()
        any_1000 = _run(eng, ids, pairs, "family_k12", mapping="anywhere")
        win_1000 = _run(eng, ids, pairs, "family_k12")
        any_500 = _run(eng, ids, pairs, "family_k12_L500", mapping="anywhere")      # the sketches are rebuilt, the index is not
        win_500 = _run(eng, ids, pairs, "family_k12_L500")
        any_again = _run(eng, ids, pairs, "family_k12", mapping="anywhere")
        old_after = old_entry()
        eng.clear_genomes()
        ids2 = _load(eng, other)      # other genomes under the same ids
        assert ids2 == ids
        win_other = _run(eng, ids2, other.pairs, "family_k16")
    assert any_1000.tobytes() == fresh_1000.tobytes() == any_again.tobytes() and any_500.tobytes() == fresh_500.tobytes()
    assert old_before.tobytes() == old_after.tobytes()
    sc.assert_records_equal(win_1000, _results("family_k12"), "window at 1000")
    sc.assert_records_equal(win_500, _results("family_k12_L500"), "window at 500")
    sc.assert_records_equal(win_other, _results("family_k16"), "window after clear_genomes")
    assert win_1000.tobytes() != any_1000.tobytes()      # (the unrelated pairs differ in `matches` at k = 12)


# ---- 6. the capacity path -----------------------------------------------------------------------------------------------------------------------
def test_reference_at_and_over_the_bin_limit():
    """A reference of more bins than one wave's LDS counters hold (8 192 at frag_len <= 65 535) is refused with PG_E_CAPACITY and the
    limit in bases; one of exactly 8 192 bins is mapped, its last bins included."""
    from pyani_amd import _lib
    from pyani_amd.engine import Engine
    case = smc.capacity()
    with Engine(0) as eng:
        ids = _load(eng, case)
        at_limit = _run(eng, ids, [(2, 0), (2, 2)], "capacity")
        with pytest.raises(_lib.PyaniGpuError) as err:
            _run(eng, ids, [(2, 2), (2, 1)], "capacity")
        assert err.value.code == _lib.PG_E_CAPACITY and str(smc.CAPACITY_LIMIT_BASES) in str(err.value) and "frag_len 64" in str(err.value)
        with pytest.raises(_lib.PyaniGpuError) as err:
            eng.sketch_pair_fragments(ids[2], ids[1], frag_len=64, scale=16, kmer=12)
        assert err.value.code == _lib.PG_E_CAPACITY
        as_query = _run(eng, ids, [(1, 2)], "capacity")      # the fragment count of a QUERY is not limited
        after = _run(eng, ids, [(2, 0), (2, 2)], "capacity")
    sc.assert_records_equal(at_limit, _results("capacity", [(2, 0), (2, 2)]), "8192 bins")
    assert int(at_limit[0]["matches"]) >= 150 and max(x[1] for x in smc.answer("capacity", 2, 0)[1]) == smc.MAX_BINS - 1
    assert int(as_query[0]["fragments"]) == smc.MAX_BINS and after.tobytes() == at_limit.tobytes()


# ---- 7. one call, many pairs -----------------------------------------------------------------------------------------------------------------------
def test_many_pairs_in_one_call_equal_single_calls_and_multiengine():
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    genomes = skc.family(12).genomes + skc.more_queries()
    pairs = [(q, r) for q in range(len(genomes)) for r in range(3)] + [(0, 3), (1, 4), (5, 4)]
    pairs = [pairs[i] for i in np.random.default_rng(17).permutation(len(pairs))]
    pairs.append(pairs[2])      # one pair twice
    kw = dict(frag_len=1000, scale=16, min_fraction=0.2, kmer=12, mapping="window")
    with Engine(0) as eng:
        ids = [eng.add_genome(s, o) for s, o in genomes]
        one = eng.sketch_pairs([ids[q] for q, _ in pairs], [ids[r] for _, r in pairs], **kw)
        single = np.concatenate([eng.sketch_pairs([ids[q]], [ids[r]], **kw) for q, r in pairs])
    with MultiEngine([0, 0]) as me:
        ids2 = [me.add_genome(s, o) for s, o in genomes]
        assert ids2 == ids
        two = me.sketch_pairs([ids[q] for q, _ in pairs], [ids[r] for _, r in pairs], **kw)
    assert one.tobytes() == single.tobytes() == two.tobytes()
    by = dict(zip(pairs, one))
    assert int(by[(0, 1)]["status"]) == 0 and int(by[(3, 0)]["status"]) == 0 and int(by[(4, 0)]["status"]) == 1 and int(by[(2, 0)]["status"]) == 1


# ---- 8. the driver ---------------------------------------------------------------------------------------------------------------------------------
def _same_run(a, b):
    assert a.results == b.results and list(a.results) == list(b.results) and a.rows == b.rows and a.lengths == b.lengths
    assert all(a.matrices[k].equals(b.matrices[k]) for k in a.matrices)


def test_run_fastani_with_the_window_mapping(synth_ci_dir, tmp_path):
    from pyani_amd import fastani
    from pyani_amd.engine import Engine
    from pyani_amd.subcmd_fastani import run_fastani
    indir = next(iter(synth_ci_dir.values())).parent
    paths = sorted(synth_ci_dir.values())
    n_pairs = len(paths) * (len(paths) - 1)
    with Engine(0) as eng:
        default_here = run_fastani(indir, kmerSize=14, engine=eng)
        first = run_fastani(indir, tmp_path, kmerSize=14, mapping="window", write_output=True, engine=eng)
        assert eng.genome_count() == 0 and len(first.written) == n_pairs and first.recovered == []
        assert sum(x is not None for x in first.results.values()) >= 2      # the set holds related genomes
        for f in first.written:      # the files parse back to the run's results
            q, r = f.name[:-len(".fastani")].split("_vs_")
            text = f.read_text()
            assert (first.results[(q, r)] is None) == (text == "")
            assert text == "" or fastani.parse_fastani_file(f) == first.results[(q, r)]
        first.written[1].unlink()
        first.written[-2].unlink()
        second = run_fastani(indir, tmp_path, kmerSize=14, mapping="window", recovery=True, write_output=True, engine=eng)
        assert len(second.written) == 2 and len(second.recovered) == n_pairs - 2
        _same_run(first, second)
        ids = [gid for gid, _, _ in eng.add_fasta_batch(paths)]
        plain = run_fastani(indir, kmerSize=14, mapping="window", engine=eng)
        direct = fastani.comparison_results(eng, paths, ids, kmerSize=14, mapping="window")
        assert plain.results == {k: v for k, v in direct.items() if k[0] != k[1]}
        for k, x in plain.results.items():      # the files hold the same estimates to 4 places of a percentage
            y = first.results[k]
            assert (x is None) == (y is None)
            assert x is None or ((x.matches, x.fragments) == (y.matches, y.fragments) and abs(x.ani - y.ani) <= 0.5e-6 + 1e-12)
        default_after = run_fastani(indir, kmerSize=14, engine=eng)
    multi = run_fastani(indir, kmerSize=14, mapping="window", devices=[0, 0])
    _same_run(plain, multi)
    with Engine(0) as eng2:      # the default mapping on an engine that never mapped
        default_fresh = run_fastani(indir, kmerSize=14, engine=eng2)
    _same_run(default_here, default_fresh)
    _same_run(default_after, default_fresh)
    assert set(plain.matrices) == set(default_fresh.matrices) and len(plain.rows) == len(default_fresh.rows) == n_pairs


# ---- 9. pricing against the exact engine ---------------------------------------------------------------------------------------------------------
def test_both_mappings_against_the_exact_engine(tmp_path):
    """The family of test_k14_estimate_against_the_exact_engine (seed 4242, 400 kb, six descendants and one unrelated genome) at
    k = 16, 14 and 12, both mappings and anim_pairs in one process.  Asserted: every pair with the unrelated genome has NO result under
    "window" at all three k; at least 20 related pairs are compared per k; the worst |window ANI - anim_pairs identity| per identity
    tier (>= 0.90, 0.80 ... 0.90, < 0.80) stays under WINDOW_BARS.  The measured errors of both mappings are written to
    sketch_map_vs_exact.json in the directory $PYANI_REPORT_DIR names (default: the test's temporary directory) and printed;
    profiles/sketch_map_vs_exact.json holds the committed copy, from which WINDOW_BARS were taken."""
    from pyani_amd import fastani, synth
    from pyani_amd.engine import Engine
    n, L = 60, 400_000
    fam = [g for g in range(n) if g % 3 == 0][:6] + [1]
    est = {}
    with Engine(0) as eng:
        ids = {g: eng.add_genome(*synth.genome(4242, n, g, L)) for g in fam}
        pairs = [(a, b) for a in fam for b in fam if a != b]
        exact = eng.anim_pairs([ids[a] for a, _ in pairs], [ids[b] for _, b in pairs])
        for k in (16, 14, 12):
            for mapping in ("anywhere", "window"):
                est[(k, mapping)] = fastani.calculate_fastani_pairs(eng, [ids[b] for _, b in pairs], [ids[a] for a, _ in pairs], kmerSize=k, mapping=mapping)
    report = {"workload": f"{len(fam) - 1} descendants of one ancestor + 1 unrelated, {L} bp, seed 4242 (bench generator), frag_len 3000, scale 16", "k": {}}
    failures = []
    for k in (16, 14, 12):
        report["k"][str(k)] = {}
        for mapping in ("anywhere", "window"):
            worst = {"hi": 0.0, "mid": 0.0, "lo": 0.0}
            count = {"hi": 0, "mid": 0, "lo": 0}
            unrelated = []
            for (a, b), x, s in zip(pairs, exact, est[(k, mapping)]):
                if a == 1 or b == 1:
                    unrelated.append((a, b, int(s["status"]), int(s["matches"]), int(s["fragments"])))
                    continue
                if int(x["status"]) or int(s["status"]):
                    continue
                tier = "hi" if float(x["identity"]) >= 0.90 else "mid" if float(x["identity"]) >= 0.80 else "lo"
                worst[tier] = max(worst[tier], abs(float(s["ani"]) - float(x["identity"])))
                count[tier] += 1
            n_cmp = sum(count.values())
            report["k"][str(k)][mapping] = {"worst_abs_error_identity_ge_0.90": worst["hi"], "worst_abs_error_identity_0.80_to_0.90": worst["mid"],
                                            "worst_abs_error_identity_lt_0.80": worst["lo"], "compared": n_cmp, "compared_per_tier": count,
                                            "unrelated_with_result": sum(st == 0 for _, _, st, _, _ in unrelated),
                                            "unrelated_matches_max": max(m for _, _, _, m, _ in unrelated), "unrelated_pairs": len(unrelated)}
            print("k =", k, mapping, "against the exact engine:", n_cmp, worst, count, "unrelated:", unrelated)
            if mapping == "window":
                bars = WINDOW_BARS[k]
                if not all(st == 1 for _, _, st, _, _ in unrelated):
                    failures.append((k, "unrelated", unrelated))
                if not (n_cmp >= 20 and worst["hi"] < bars[0] and worst["mid"] < bars[1] and worst["lo"] < bars[2]):
                    failures.append((k, n_cmp, worst, bars))
    report_dir = Path(os.environ.get("PYANI_REPORT_DIR") or tmp_path)
    report_dir.mkdir(parents=True, exist_ok=True)
    (report_dir / "sketch_map_vs_exact.json").write_text(json.dumps(report, indent=1))
    assert not failures, failures


# worst |error| of "window" per tier (>= 0.90, 0.80 ... 0.90, < 0.80) measured on MI355X (profiles/sketch_map_vs_exact.json) times 1.25,
# rounded up to two significant digits; the results are bit-deterministic, the margin is for a change of the family's genomes
# measured worst errors: k = 16: 0.003858 / 0.015972 / 0.028158; k = 14: 0.004201 / 0.014724 / 0.024729; k = 12: 0.005321 / 0.014036 / 0.020472
# ("anywhere" in the same run: 0.0071 / 0.0165 / 0.0287; 0.0078 / 0.0184 / 0.0277; 0.0172 / 0.0518 / 0.0576)
WINDOW_BARS = {16: (0.0049, 0.020, 0.036), 14: (0.0053, 0.019, 0.031), 12: (0.0067, 0.018, 0.026)}
