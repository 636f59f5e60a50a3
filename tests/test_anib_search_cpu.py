"""The ANIb search mode (pg_anib_set_search: "seeds" | "all_diagonals") without a GPU: the yardstick the GPU tests use — the host
statement of fragment mode in both modes against the independent blastn oracle — gives the agreement counts the mode was specified
with; the ABI's two calls are declared, bound and exported; unknown names and a recovery across modes are refused before any device
is touched."""
import json
import re

import pytest

from tests import anib_search_cases as cases
from tests.conftest import ROOT

# (query, subject): (used rows of the oracle, identical in default mode, identical with every diagonal walked)
TABLE = {(5, 4): (132, 121, 130), (4, 5): (125, 120, 124), (3, 5): (128, 125, 127)}


@pytest.mark.parametrize("pair", sorted(TABLE))
def test_host_statement_agreement_counts(monkeypatch, pair):
    used, default, every = TABLE[pair]
    assert cases.oracle_agreement(cases.host_rows(monkeypatch, *pair, "seeds"), *pair) == (used, default)
    assert cases.oracle_agreement(cases.host_rows(monkeypatch, *pair, "all_diagonals"), *pair) == (used, every)


@pytest.mark.parametrize("pair", cases.CLOSE)
def test_host_statement_mode_changes_nothing_on_close_pairs(monkeypatch, pair):
    a, b = cases.host_rows(monkeypatch, *pair, "seeds"), cases.host_rows(monkeypatch, *pair, "all_diagonals")
    assert cases.rows_of(a) == cases.rows_of(b) and len(a) > 100


def test_abi_declares_binds_and_exports_the_setting():
    from pyani_amd import build, _lib
    build.build_gpu()
    lib = _lib.load()
    header = (ROOT / "include" / "pyani_gpu.h").read_text()
    for sym in ("pg_anib_set_search", "pg_anib_get_search"):
        assert re.search(rf"\b{sym}\s*\(", header) and sym in _lib.SIGNATURES and hasattr(lib, sym)
    assert len(_lib.SIGNATURES["pg_anib_set_search"][1]) == 2 and len(_lib.SIGNATURES["pg_anib_get_search"][1]) == 2
    assert re.search(r"#define PG_ANIB_SEARCH_SEEDS 0u?\b", header) and re.search(r"#define PG_ANIB_SEARCH_ALL_DIAGS 1u?\b", header)
    assert _lib.ANIB_SEARCH_MODES == {"seeds": 0, "all_diagonals": 1}
    # the calls that read the setting keep their signatures
    assert [len(_lib.SIGNATURES[s][1]) for s in ("pg_anib_pairs", "pg_anib_pair_rows", "pg_anib_rows_batch")] == [6, 7, 7]
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    for cls in (Engine, MultiEngine):
        assert callable(getattr(cls, "anib_set_search")) and isinstance(getattr(cls, "anib_search"), property)


class NoEngine:      # any use of the engine is a library call
    def __getattr__(self, name):
        raise AssertionError(f"engine touched: {name}")


def test_unknown_mode_is_a_value_error_before_any_library_call(tmp_path):
    from pyani_amd import anib, subcmd_anib as sa
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    for bad in ("bogus", "", "SEEDS", None, 1):
        with pytest.raises(ValueError):
            Engine.anib_set_search(NoEngine(), bad)
        with pytest.raises(ValueError):
            MultiEngine.anib_set_search(NoEngine(), bad)
    with pytest.raises(ValueError, match="bogus"):
        sa.run_anib(tmp_path, None, engine=NoEngine(), search="bogus")
    with pytest.raises(ValueError, match="bogus"):
        anib.calculate_anib_pairs([], engine=NoEngine(), search="bogus")
    with pytest.raises(ValueError):
        with anib.search_mode(NoEngine(), "bogus"):
            pass


def test_recovery_across_modes_is_refused_without_a_device(tmp_path):
    from pyani_amd import subcmd_anib as sa
    out = tmp_path / "out"
    out.mkdir()
    assert sa.recorded_search(out) == "seeds"      # no record: the default search (BLAST+'s own tables, earlier runs)
    with pytest.raises(ValueError, match="all_diagonals"):
        sa.run_anib(tmp_path / "in", out, recovery=True, search="all_diagonals", engine=NoEngine())
    (out / sa.RUN_RECORD).write_text(json.dumps({"search": "all_diagonals", "fragsize": 1020}))
    assert sa.recorded_search(out) == "all_diagonals"
    with pytest.raises(ValueError, match="seeds"):
        sa.run_anib(tmp_path / "in", out, recovery=True, engine=NoEngine())      # the default keyword is "seeds"
    with pytest.raises(ValueError, match="seeds"):
        sa.run_anib(tmp_path / "in", out, recovery=True, search="seeds", engine=NoEngine())


class FakeEngine:
    """Records the mode changes; fails inside the body when told to."""
    def __init__(self):
        self.mode, self.log = "seeds", []

    @property
    def anib_search(self):
        return self.mode

    def anib_set_search(self, mode):
        self.mode = mode
        self.log.append(mode)


def test_search_mode_is_restored_on_the_way_out_on_errors_too():
    from pyani_amd import anib
    e = FakeEngine()
    with anib.search_mode(e, "all_diagonals"):
        assert e.mode == "all_diagonals"
    assert e.mode == "seeds" and e.log == ["all_diagonals", "seeds"]
    e.mode = "all_diagonals"      # the caller's own setting comes back, not the default
    with pytest.raises(RuntimeError):
        with anib.search_mode(e, "seeds"):
            assert e.mode == "seeds"
            raise RuntimeError("inside")
    assert e.mode == "all_diagonals"
