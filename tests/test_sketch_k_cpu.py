"""CPU: the sketch mode for k-mer sizes 8 ... 16 (pyani_amd/csrc/pg_sketch_core.h) — the numpy statement with k as a parameter
(tests/sketch_k_cases.py) tied to the pinned k = 16 oracle, the root of the general case against a 60-digit decimal root, the host
statement against numpy bit for bit (tests/sketch_k/identity_check.cpp, also under the address / undefined-behaviour sanitizers),
the non-vacuity of the GPU cases on the definition alone, and the Python layer (fastani, run_fastani, MultiEngine.sketch_pairs) on
stub engines.  Interface replaced: pyani/fastani.py, pyani/scripts/subcommands/subcmd_fastani.py:114-480."""
import decimal
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import sketch_cases as sc
from tests import sketch_k_cases as skc
from tests.conftest import ROOT


# ---- 1. k = 16 equals the pinned oracle ----------------------------------------------------------------------------------------------
def test_k16_of_the_helper_equals_the_pinned_oracle():
    import sketch_oracle as so
    rng = np.random.default_rng(20261001)
    off = sc.offsets(120_000, 3, 23)
    a = sc.random_bases(rng, 120_000)
    genomes = [(a, off), (sc.substituted(rng, a), off), (sc.random_bases(rng, 120_000), off)]
    for frag_len, scale, minfrac in ((3000, 16, 0.2), (1000, 4, 0.5)):
        old = [so.genome_sketch(s, o, frag_len=frag_len, scale=scale) for s, o in genomes]
        new = [skc.genome_sketch(s, o, 16, frag_len=frag_len, scale=scale) for s, o in genomes]
        for x, y in zip(old, new):
            assert x[0] == y[0] and x[2] == y[2] and all((f == g).all() for f, g in zip(x[1], y[1]))
        n_ok = 0
        for q in range(3):
            for r in range(3):
                want = so.sketch_pair(old[q], old[r], minfrac)
                got = skc.sketch_pair(new[q], new[r], 16, minfrac)
                assert got[1:] == want[1:] and float(got[0]).hex() == float(want[0]).hex(), (q, r, got, want)
                n_ok += want[3] == 0
        assert n_ok == 5      # the family's four pairs and the unrelated genome against itself
    h, n = skc.identity_grid()
    four = np.sqrt(np.sqrt(np.sqrt(np.sqrt(h / n))))
    assert (skc.frag_identity(h, n, 16).view(np.uint64) == four.view(np.uint64)).all()


# ---- 2. the root -----------------------------------------------------------------------------------------------------------------------
def _decimal_root(h, n, k, ctx):
    """(h / n)^(1/k) to 60 digits: Newton in decimal arithmetic from a float start (quadratic: 15 digits -> 30 -> 60; the third step is the margin)."""
    c = ctx.divide(decimal.Decimal(h), decimal.Decimal(n))
    y = decimal.Decimal((h / n) ** (1.0 / k))
    kd = decimal.Decimal(k)
    for _ in range(3):
        p = ctx.power(y, k - 1)
        y = ctx.subtract(y, ctx.divide(ctx.subtract(ctx.multiply(p, y), c), ctx.multiply(kd, p)))
    return y


def test_the_root_is_within_one_ulp_of_a_60_digit_decimal_root():
    ctx = decimal.Context(prec=60)
    h, n = skc.identity_grid()
    g = np.gcd(h, n)
    # frag_identity sees h / n only: one decimal root per distinct fraction
    frac, first = np.unique(np.stack([h // g, n // g], axis=1), axis=0, return_index=True)
    floor = decimal.Decimal(skc.MIN_IDENTITY)      # the double 0.80, exactly
    worst, near_floor = 0.0, []
    for k in range(8, 16):
        got = skc.frag_identity(h, n, k)
        assert (got[h == n] == 1.0).all()
        assert (got.view(np.uint64) == skc.frag_identity(h // g, n // g, k).view(np.uint64)).all()
        for (a, b), i in zip(frac.tolist(), first.tolist()):
            y = float(got[i])
            root = _decimal_root(a, b, k, ctx)
            ulp = decimal.Decimal(float(np.spacing(y)))
            err = abs(decimal.Decimal(y) - root) / ulp
            worst = max(worst, float(err))
            assert err <= 1, (k, a, b, y, root)
            if abs(root - floor) <= decimal.Decimal(float(np.spacing(skc.MIN_IDENTITY))):
                near_floor.append((k, a, b))
            else:
                assert (y >= skc.MIN_IDENTITY) == (root >= floor), (k, a, b, y, root)
    print("worst error of the root:", worst, "ulp; exact root within 1 ulp of 0.80:", near_floor)
    assert near_floor == []      # none is expected


# ---- 3. the host statement = numpy, bit for bit (and clean under the sanitizers) -----------------------------------------------------------
def _check_record():
    rng = np.random.default_rng(20261003)
    seq = sc.random_bases(rng, 4_000)
    seq[500:503] = ord("N")
    seq[1_000:1_040] = ord("n")
    seq[2_000:2_200] = np.frombuffer(bytes(seq[2_000:2_200]).lower(), dtype=np.uint8)
    seq[3_990] = ord("R")
    return seq


def _expected_lines(seq):
    h, n = skc.identity_grid()
    lines = []
    for k in (8, 11, 15, 16):
        bits = skc.frag_identity(h, n, k).view(np.uint64)
        lines += [f"I {k} {a} {b} {x:016x}" for a, b, x in zip(h.tolist(), n.tolist(), bits.tolist())]
        pos, fwd, rc = skc.record_words(seq, k)
        canon = np.minimum(fwd, rc)
        smp = (skc.mix32(canon.copy()) & np.uint64(15)) == 0      # (the oracle's mix32 works in place on a uint64 array)
        lines += [f"W {k} {p} {f:08x} {r:08x} {c:08x} {int(s)}" for p, f, r, c, s in zip(pos.tolist(), fwd.tolist(), rc.tolist(), canon.tolist(), smp.tolist())]
    return lines


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_host_statement_equals_numpy_bit_for_bit(tmp_path, sanitize):
    src = ROOT / "tests" / "sketch_k" / "identity_check.cpp"
    exe = tmp_path / "identity_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(src), "-o", str(exe)],
                   check=True)
    seq = _check_record()
    rec = tmp_path / "record.txt"
    rec.write_bytes(bytes(seq) + b"\n")
    out = subprocess.run([str(exe), str(rec)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    got, want = out.stdout.splitlines(), _expected_lines(seq)
    assert len(got) == len(want) and sum(ln.startswith("W ") for ln in want) > 4 * 3_000
    bad = [(g, w) for g, w in zip(got, want) if g != w]
    assert not bad, bad[:5]


# ---- 4. the GPU cases say something (on the definition alone) -----------------------------------------------------------------------------
@pytest.mark.parametrize("k,size,frag_len,scale,minfrac", skc.K_PARAMS)
def test_gpu_cases_are_not_vacuous(k, size, frag_len, scale, minfrac):
    fn = skc.case_fn("family", k)
    case = fn()
    want = skc.k_pairs(fn, k, frag_len, scale, minfrac)
    strong, related, unrelated = sc.non_vacuity(case, want)
    print(k, [(p, w[1], w[2]) for p, w in zip(case.pairs, want)])
    # (0, 0), (0, 1), (1, 0), (1, 1) and the unrelated genome against itself: every one of them strong; four unrelated pairs without a result
    assert (strong, related, unrelated) == (5, 5, 4)
    if k <= 11:      # the unrelated pairs have matches of their own: the hit counts are a real comparison
        assert any(w[1] > 0 for p, w in zip(case.pairs, want) if p not in case.related)


@pytest.mark.parametrize("k", [8, 15])
def test_record_cases_are_not_vacuous(k):
    fn = skc.case_fn("records", k)
    want = skc.k_pairs(fn, k, 64, 16, 0.2)
    assert sc.non_vacuity(fn(), want) == (4, 4, 0)
    lengths = fn().lengths
    assert {k - 1, k, k + 1, 63 + k, 64 + k} <= set(lengths) and lengths[0] == 0 and lengths[-1] == 0


def test_extreme_scales_at_k12_are_not_vacuous():
    """(frag_len 65, scale 1): every k-mer is sampled, every related pair is strong.  (frag_len 3000, scale 4096): ~30 sampled k-mers in
    the whole genome — few fragments can match, no pair reaches min_fraction; what is compared is the matching fragments' count."""
    f12 = skc.case_fn("family", 12)
    assert sc.non_vacuity(f12(), skc.k_pairs(f12, 12, 65, 1, 0.2)) == (5, 5, 4)
    want = skc.k_pairs(f12, 12, 3000, 4096, 0.2)
    by = dict(zip(f12().pairs, want))
    assert all(w[1] == 0 and w[3] == 1 for p, w in by.items() if p not in f12().related)
    assert by[(0, 0)][1] >= 2 and by[(1, 1)][1] >= 2 and by[(0, 0)][2] == 39


# ---- 5. the Python layer without a GPU ---------------------------------------------------------------------------------------------------
class StubEngine:
    """Records its sketch_pairs calls; answers from a table {(query id, reference id): (ani, matches, fragments, status)}."""

    def __init__(self, table=None, lengths=None):
        self.calls, self.table, self.lengths, self.n, self.cleared = [], table or {}, lengths or [], 0, 0

    def sketch_pairs(self, qry_ids, ref_ids, frag_len=3000, scale=16, min_fraction=0.2, kmer=16):
        from pyani_amd.engine import Engine
        self.calls.append({"q": [int(x) for x in qry_ids], "r": [int(x) for x in ref_ids], "frag_len": frag_len, "scale": scale, "min_fraction": min_fraction,
                           "kmer": kmer})
        out = np.zeros(len(self.calls[-1]["q"]), dtype=Engine.SKETCH_DTYPE)
        for i, key in enumerate(zip(self.calls[-1]["q"], self.calls[-1]["r"])):
            ani, m, f, st = self.table.get(key, (0.5 + 0.01 * key[0] + 0.001 * key[1], 10 * key[0] + key[1], 100, 0))
            out[i] = (ani, m, f, st, 0)
        return out

    def genome_count(self):
        return self.n

    def add_fasta_batch(self, paths, threads=0):
        first = self.n
        self.n += len(paths)
        return [(first + i, self.lengths[i], 1) for i in range(len(paths))]

    def clear_genomes(self):
        self.cleared += 1
        self.n = 0


def test_fastani_functions_pass_the_kmer_size_on():
    from pyani_amd import fastani
    stub = StubEngine()
    fastani.calculate_fastani_pairs(stub, [0, 1], [1, 0], kmerSize=12)
    assert stub.calls[-1]["kmer"] == 12 and stub.calls[-1]["frag_len"] == 3000 and stub.calls[-1]["min_fraction"] == 0.2
    fastani.calculate_fastani_pairs(stub, [0], [1])
    assert stub.calls[-1]["kmer"] == 16
    res = fastani.comparison_results(stub, [Path("a.fna"), Path("b.fna")], [0, 1], fragLen=1000, kmerSize=9, minFraction=0.3)
    assert stub.calls[-1]["kmer"] == 9 and stub.calls[-1]["frag_len"] == 1000 and stub.calls[-1]["min_fraction"] == 0.3 and len(res) == 4
    n = len(stub.calls)
    for bad in (7, 17):
        with pytest.raises(fastani.PyaniFastANIException):
            fastani.calculate_fastani_pairs(stub, [0], [1], kmerSize=bad)
        with pytest.raises(fastani.PyaniFastANIException):
            fastani.comparison_results(stub, [Path("a.fna")], [0], kmerSize=bad)
    assert len(stub.calls) == n      # refused before the engine is touched
    row = fastani.comparison_row(fastani.ComparisonResult("q.fna", "r.fna", 0.9, 12, 20), "q.fna", "r.fna", 3000, 90_000, kmerSize=12, minFraction=0.3)
    assert (row["kmersize"], row["minmatch"]) == (12, 0.3)
    row = fastani.comparison_row(None, "q.fna", "r.fna", 3000, 90_000)
    assert (row["kmersize"], row["minmatch"], row["aln_length"]) == (16, 0.2, 0)


def _write_inputs(d):
    rng = np.random.default_rng(5)
    lengths = {"a": 700, "b": 650, "c": 900}
    for stem, n in lengths.items():
        (d / f"{stem}.fna").write_text(f">{stem}\n{bytes(sc.random_bases(rng, n)).decode()}\n")
    return lengths


def test_run_fastani_on_a_stub_engine(tmp_path):
    from pyani_amd import fastani
    from pyani_amd.subcmd_fastani import run_fastani
    indir = tmp_path / "in"
    indir.mkdir()
    lengths = _write_inputs(indir)
    stems = ["a", "b", "c"]
    frag = 100
    table = {(0, 1): (0.987654321, 5, 7, 0), (0, 2): (0.0, 1, 7, 1), (1, 0): (0.91, 6, 6, 0), (1, 2): (0.8512345, 2, 6, 0), (2, 0): (0.0, 0, 9, 1), (2, 1): (0.95, 9, 9, 0)}
    order = [(q, r) for q in stems for r in stems if q != r]
    for kw in ({"write_output": True}, {"recovery": True}):
        with pytest.raises(ValueError):
            run_fastani(indir, **kw, engine=StubEngine(table, [700, 650, 900]))
    with pytest.raises(fastani.PyaniFastANIException):
        run_fastani(indir, kmerSize=17, engine=StubEngine(table, [700, 650, 900]))
    (indir / "sub").mkdir()

    # a run that writes nothing: the engine's values
    stub = StubEngine(table, [700, 650, 900])
    plain = run_fastani(indir, fragLen=frag, kmerSize=12, minFraction=0.3, engine=stub)
    assert len(stub.calls) == 1 and stub.calls[0]["kmer"] == 12 and stub.calls[0]["frag_len"] == frag and stub.calls[0]["min_fraction"] == 0.3
    assert list(zip(stub.calls[0]["q"], stub.calls[0]["r"])) == [(stems.index(q), stems.index(r)) for q, r in order]
    assert stub.cleared == 1      # the genomes this call added to an empty engine are gone
    assert list(plain.results) == order and plain.lengths == lengths and plain.recovered == [] and plain.written == []
    assert plain.results[("a", "b")] == fastani.ComparisonResult(indir / "a.fna", indir / "b.fna", 0.987654321, 5, 7)
    assert plain.results[("a", "c")] is None and plain.results[("c", "a")] is None

    # a run that writes: file names, contents, results = the files read back
    out = tmp_path / "out"
    stub = StubEngine(table, [700, 650, 900])
    first = run_fastani(indir, out, fragLen=frag, kmerSize=12, minFraction=0.3, write_output=True, engine=stub)
    assert first.written == [out / "fastani_output" / f"{q}_vs_{r}.fastani" for q, r in order]
    assert sorted(p.name for p in (out / "fastani_output").iterdir()) == sorted(f"{q}_vs_{r}.fastani" for q, r in order)
    for (q, r), f in zip(order, first.written):
        key = (stems.index(q), stems.index(r))
        if table[key][3]:
            assert f.read_text() == "" and first.results[(q, r)] is None
        else:
            assert f.read_text() == f"{indir / (q + '.fna')}\t{indir / (r + '.fna')}\t{100.0 * table[key][0]:.4f}\t{table[key][1]}\t{table[key][2]}\n"
            back = fastani.parse_fastani_file(f)
            assert back == first.results[(q, r)] and back[:2] == (str(indir / f"{q}.fna"), str(indir / f"{r}.fna"))
            assert abs(back.ani - table[key][0]) <= 0.5e-6 + 1e-12 and (back.matches, back.fragments) == table[key][1:3]

    # rows and matrices, cell for cell
    assert [(row["query"], row["subject"]) for row in first.rows] == [
        (str(indir / f"{q}.fna"), str(indir / f"{r}.fna")) if first.results[(q, r)] else (indir / f"{q}.fna", indir / f"{r}.fna") for q, r in order]
    for run in (plain, first):
        m = run.matrices
        assert set(m) == {"identity", "coverage", "aln_lengths", "sim_errors", "hadamard"}
        for name, diag in (("identity", 1.0), ("coverage", 1.0), ("sim_errors", 0.0), ("hadamard", 1.0)):
            assert [m[name].loc[s, s] for s in stems] == [diag] * 3
        assert [m["aln_lengths"].loc[s, s] for s in stems] == [float(lengths[s]) for s in stems]
        for (q, r), row in zip(order, run.rows):
            res = run.results[(q, r)]
            ani, matches, frags = (res.ani, res.matches, res.fragments) if res else (0.0, 0, 0)
            cov = float(matches) * frag / lengths[q]
            assert (row["identity"], row["cov_query"], row["aln_length"], row["sim_errs"]) == (ani, cov, matches * frag, (frags - matches) * frag)
            assert (row["kmersize"], row["minmatch"], row["fragsize"], row["program"]) == (12, 0.3, frag, "fastANI")
            cell = [m[name].loc[q, r] for name in ("identity", "coverage", "aln_lengths", "sim_errors", "hadamard")]
            assert cell == [ani, cov, matches * frag, (frags - matches) * frag, ani * cov], (q, r)
            assert list(m["identity"].index) == stems and list(m["identity"].columns) == stems

    # recovery: exactly the existing files are skipped, an empty one included
    (out / "fastani_output" / "a_vs_b.fastani").unlink()
    (out / "fastani_output" / "c_vs_a.fastani").unlink()        # (an empty file: a result the engine is asked for again)
    stub = StubEngine(table, [700, 650, 900])
    second = run_fastani(indir, out, fragLen=frag, kmerSize=12, minFraction=0.3, recovery=True, write_output=True, engine=stub)
    assert len(stub.calls) == 1 and list(zip(stub.calls[0]["q"], stub.calls[0]["r"])) == [(0, 1), (2, 0)]
    assert [p.name for p in second.written] == ["a_vs_b.fastani", "c_vs_a.fastani"]
    assert [p.name for p in second.recovered] == ["a_vs_c.fastani", "b_vs_a.fastani", "b_vs_c.fastani", "c_vs_b.fastani"]      # a_vs_c is empty
    assert second.results == first.results and list(second.results) == order and second.rows == first.rows
    assert all(second.matrices[k].equals(first.matrices[k]) for k in first.matrices)
    stub = StubEngine(table, [700, 650, 900])
    third = run_fastani(indir, out, fragLen=frag, kmerSize=12, minFraction=0.3, recovery=True, engine=stub)
    assert stub.calls == [] and len(third.recovered) == 6 and third.results == first.results

    # duplicate stems
    (indir / "a.fasta").write_text(">x\nACGT\n")
    with pytest.raises(ValueError):
        run_fastani(indir, engine=StubEngine(table, [4, 700, 650, 900]))


def test_multiengine_sketch_pairs_deals_by_query_and_restores_call_order():
    from pyani_amd.multi import MultiEngine
    me = MultiEngine.__new__(MultiEngine)      # (no device: the engines are stubs)
    me.devices, me.engines, me.chunk_pairs, me.last_chunks_per_engine = [0, 1, 2], [StubEngine(), StubEngine(), StubEngine()], 0, []
    rng = np.random.default_rng(11)
    pairs = [(q, r) for q in range(7) for r in range(7) if q != r and (q + r) % 3]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))] + [pairs[0]]
    q, r = [a for a, _ in pairs], [b for _, b in pairs]
    res = me.sketch_pairs(q, r, 1000, 4, 0.5, 12)
    one = StubEngine().sketch_pairs(q, r, 1000, 4, 0.5, 12)
    assert res.tobytes() == one.tobytes()      # the records in call order
    seen = []
    for e in me.engines:
        assert len(e.calls) == 1      # one call per device
        c = e.calls[0]
        assert (c["frag_len"], c["scale"], c["min_fraction"], c["kmer"]) == (1000, 4, 0.5, 12)
        seen.append(set(c["q"]))
    assert not (seen[0] & seen[1]) and not (seen[0] & seen[2]) and not (seen[1] & seen[2])      # a query's pairs stay on one device
    assert sorted(p for e in me.engines for p in zip(e.calls[0]["q"], e.calls[0]["r"])) == sorted(pairs)
    sizes = [len(e.calls[0]["q"]) for e in me.engines]
    assert max(sizes) - min(sizes) <= 6      # (no share is more than one query's pairs ahead)
    assert len(me.sketch_pairs([], [])) == 0
    with pytest.raises(ValueError):
        me.sketch_pairs([0, 1], [1])


def test_library_exports_the_general_k_entry():
    from pyani_amd import _lib, build
    build.build_gpu()
    lib = _lib.load()
    assert hasattr(lib, "pg_sketch_pairs_k") and hasattr(lib, "pg_sketch_pairs")
    assert "pg_sketch_pairs_k" in _lib.SIGNATURES and len(_lib.SIGNATURES["pg_sketch_pairs_k"][1]) == len(_lib.SIGNATURES["pg_sketch_pairs"][1]) + 1
