"""The host side of the batched ANIb tables: the ABI's two calls are exported and declared, the multi-device merge puts parts back
into the caller's order, run_anib's path helpers give the legacy script's names."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests.conftest import ROOT


def test_abi_exports_and_declares_the_rows_calls():
    from pyani_amd import build, _lib
    build.build_gpu()
    lib = _lib.load()
    header = (ROOT / "include" / "pyani_gpu.h").read_text()
    for sym in ("pg_anib_rows_batch", "pg_anib_rows_read"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert len(_lib.SIGNATURES["pg_anib_rows_batch"][1]) == 7 and len(_lib.SIGNATURES["pg_anib_rows_read"][1]) == 2
    # the two passes have profile slots after the published range; index 20 (= PG_K__COUNT) is no slot
    assert (_lib.K_ANIB_ROWS_SCAN, _lib.K_ANIB_ROWS_PACK, _lib.K_END) == (21, 22, 23)
    assert re.search(r"#define PG_K_ANIB_ROWS_SCAN 21\b", header) and re.search(r"#define PG_K_ANIB_ROWS_PACK 22\b", header)
    assert re.search(r"#define PG_K__END 23\b", header)
    assert lib.pg_kernel_name(21) == b"anib_rows_scan_kernels" and lib.pg_kernel_name(22) == b"anib_rows_pack_kernel"
    assert lib.pg_kernel_name(20) == b"" and lib.pg_kernel_name(23) == b""
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    for cls in (Engine, MultiEngine):
        assert callable(getattr(cls, "anib_rows_batch"))


def _part(engine_cls, counts, tag):
    """A fake Engine.anib_rows_batch result over len(counts) pairs: pair j has counts[j] rows whose `score` is tag * 1000 + j."""
    res = np.zeros(len(counts), dtype=engine_cls.ANIB_DTYPE)
    res["n_frags"] = [tag * 1000 + j for j in range(len(counts))]
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(counts)
    rows = np.zeros(int(off[-1]), dtype=engine_cls.ANIB_ROW_DTYPE)
    for j, c in enumerate(counts):
        rows["score"][int(off[j]):int(off[j + 1])] = tag * 1000 + j
        rows["frag"][int(off[j]):int(off[j + 1])] = np.arange(c)
    return res, off, rows


def test_merge_puts_shuffled_parts_back_into_caller_order():
    from pyani_amd.engine import Engine
    from pyani_amd.multi import merge_anib_row_parts
    n = 11
    perm = np.random.RandomState(2).permutation(n)
    chunks = [perm[:4], np.zeros(0, dtype=np.int64), perm[4:5], perm[5:]]      # an empty part among them
    counts = [[3, 0, 2, 1], [], [0], [5, 0, 0, 4, 1, 2]]                     # 0-row pairs, a part without any row
    parts = [_part(Engine, c, t) for t, c in enumerate(counts)]
    res, off, rows = merge_anib_row_parts(n, chunks, parts)
    assert res.dtype == Engine.ANIB_DTYPE and rows.dtype == Engine.ANIB_ROW_DTYPE and off.dtype == np.uint64
    assert len(off) == n + 1 and off[0] == 0 and int(off[-1]) == len(rows) == sum(sum(c) for c in counts)
    for t, (idx, c) in enumerate(zip(chunks, counts)):
        for j, p in enumerate(idx):
            mine = rows[int(off[p]):int(off[p + 1])]
            assert len(mine) == c[j] and (mine["score"] == t * 1000 + j).all() and mine["frag"].tolist() == list(range(c[j]))
            assert int(res[p]["n_frags"]) == t * 1000 + j
    empty = merge_anib_row_parts(0, [], [])
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and len(empty[2]) == 0


def test_path_helpers_give_the_legacy_names():
    from pyani_amd import subcmd_anib as sa
    out = Path("/x/out")
    assert sa.ALIGNDIR == "blastn_output"
    assert sa.table_path(out, "GCF_000011745.1_ASM1174v1_genomic", "NC_002696") == \
        out / "blastn_output" / "GCF_000011745.1_ASM1174v1_genomic_vs_NC_002696.blast_tab"
    assert sa.table_path(out, "a.b", "c.d.e").name == "a.b_vs_c.d.e.blast_tab"
    assert sa.fragment_path(out, Path("/in/GCF_000011745.1_ASM1174v1_genomic.fna")) == \
        out / "blastn_output" / "GCF_000011745.1_ASM1174v1_genomic-fragments.fna"
    assert sa.fragment_path(out, "/in/a.b.fasta").name == "a.b-fragments.fasta"


def test_run_anib_refuses_missing_outdir_before_any_work(tmp_path):
    from pyani_amd import subcmd_anib as sa

    class NoEngine:      # any use of the engine is work
        def __getattr__(self, name):
            raise AssertionError(f"engine touched: {name}")
    for kw in (dict(write_output=True), dict(recovery=True)):
        with pytest.raises(ValueError):
            sa.run_anib(tmp_path / "does-not-exist", None, engine=NoEngine(), **kw)


def test_row_bookkeeping_under_the_sanitizers(tmp_path):
    """The host code that files the launches' packed rows and puts them back into the caller's order (pg_anib_rows.h), as a
    stand-alone program built with the address and undefined-behaviour sanitizers."""
    import subprocess
    exe = tmp_path / "rows_merge_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{ROOT / 'pyani_amd' / 'csrc'}", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "anib_rows" / "rows_merge_check.cpp"),
                    "-o", str(exe), "-lpthread"], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "WRONG" not in run.stdout and run.stdout.count("ok ") == 6, run.stdout + run.stderr
