"""CPU-only: the mapped sketch mode's definition (tests/sketch_map_cases.py) does what it is meant to do on the cases the GPU tests
use — so that "the GPU equals the definition" (tests/test_sketch_map_gpu.py) means something — it agrees with today's definition where
the two must agree, and the new entry points are bound."""
import re
from pathlib import Path

import pytest

from tests import sketch_map_cases as smc

ROOT = Path(__file__).resolve().parent.parent
R = smc.RULES


# ---- 1. the definition is not vacuous -----------------------------------------------------------------------------------------------------
def test_mapping_removes_chance_hits_and_repeated_copies():
    res = {name: smc.answer("rules", R[q], R[r]) for name, (q, r) in
           dict(ba=("b", "a"), ua=("u", "a"), au=("a", "u"), bsh=("b", "sh"), dupa=("dup", "a"), adup=("a", "dup"), aa=("a", "a")).items()}
    for q, r in (("u", "a"), ("a", "u")):      # unrelated: today every fragment matches on chance hits anywhere; mapped: nothing
        ani, matches, frags, status = smc.anywhere("rules", R[q], R[r])
        assert status == 0 and matches == frags == 240 and 0.84 < ani < 0.87
        assert smc.answer("rules", R[q], R[r])[0] == (0.0, 0, 240, 1)
    assert res["aa"][0] == (1.0, 240, 240, 0)
    assert abs(res["ba"][0][0] - 0.97) < 0.002 and res["ba"][0][1:] == (240, 240, 0)      # a 3 % copy: every fragment, the true identity
    # the triplicated 20 kb: one copy's 40 fragments survive, the other 80 lose their bins; the single-copy 40 kb keeps its 80
    (ani, matches, frags, status), recs, stats = res["dupa"]
    assert (ani, matches, frags, status) == (1.0, 120, 200, 0) and stats["dropped"] == 80
    kept = [f for f, r in enumerate(recs) if r[5]]
    assert kept == list(range(40)) + list(range(120, 200))      # ties go to the lowest fragment index: the FIRST copy
    assert smc.anywhere("rules", R["dup"], R["a"])[1] == 200    # (today all three copies count)
    # halves moved far apart: a window holds half a fragment
    assert res["bsh"][0][1] < res["ba"][0][1] and res["bsh"][0][0] < res["ba"][0][0]
    assert res["bsh"][0][1:] == (178, 240, 0)


def test_every_rule_of_the_definition_is_used_by_the_cases():
    """The counts over all sets but the capacity one (pinned: an edit of a case cannot silently remove a rule).  window_tie: fragments
    whose maximum is reached by several windows (the lowest is taken); bin_up: bin = w* + 1; dropped: candidates that lose their bin;
    identity_tie: of those, with the winner's identity (the lower index won); low_identity: h >= 2 below 0.80; few_hits: h < 2;
    list_overflow: fragments that touch more bins than the mapping kernel lists."""
    assert smc.total_stats() == {"window_tie": 12837, "bin_up": 14150, "dropped": 730, "identity_tie": 632, "low_identity": 629, "few_hits": 3883,
                                 "list_overflow": 10}
    for name in ("family_k8", "family_k12", "family_k16"):      # the sets themselves: related pairs map, unrelated ones do not
        case = smc.SETS[name][0]()
        for (q, r), (res, _, _) in zip(case.pairs, smc.answers(name)):
            assert (res[3] == 0 and 2 * res[1] >= res[2]) == ((q, r) in case.related), (name, q, r, res)
    assert [a[0][2] for a in smc.answers("edges", [(4, 3), (5, 3)])] == [0, 1]      # no fragment; one fragment, all N
    assert smc.answer("edges", 5, 3)[1] == [(-1, -1, 0, 0, 0.0, 0)]
    assert [smc._bins("edges", g)[1] for g in range(4)] == [1, 1, 2, 2]
    assert smc._bins("capacity", 0)[1] == smc.MAX_BINS and smc._bins("capacity", 1)[1] == smc.MAX_BINS + 1


# ---- 2. consistency and binding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q,r", [(1, 0), (1, 1), (2, 0), (2, 1), (3, 4)])
def test_one_bin_and_one_candidate_is_todays_definition(q, r):
    """A reference of ONE bin has one window: every hit lies in it, so h is the plain hit count; with at most one candidate fragment
    the one-per-bin rule drops nothing — the mapped answer is today's."""
    bins, nb = smc._bins("edges", r)
    assert nb == 1
    res, recs, stats = smc.answer("edges", q, r)
    assert sum(x[4] >= smc.MIN_IDENTITY for x in recs) <= 1 and stats["dropped"] == 0
    rset = smc._frags("edges", r)[0]
    assert [x[2] for x in recs] == [sum(int(v) in rset for v in occ) for occ in smc._frags("edges", q)[1]]
    assert res == smc.anywhere("edges", q, r) and res[3] == 0


def _header_arity(name):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pyani_gpu.h").read_text(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/pyani_gpu.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_are_declared_and_bound():
    from pyani_amd import _lib
    for name, arity in (("pg_sketch_pairs_mapped", 9), ("pg_sketch_pair_fragments", 9), ("pg_sketch_map_last_ms", 2)):
        assert _header_arity(name) == arity == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["pg_sketch_pairs_mapped"] == _lib.SIGNATURES["pg_sketch_pairs_k"]      # the same arguments and result struct
    text = (ROOT / "include" / "pyani_gpu.h").read_text()
    assert "} pg_sketch_fragment;" in text
    from pyani_amd.engine import Engine
    assert Engine.SKETCH_FRAGMENT_DTYPE.itemsize == 32
    assert Engine.SKETCH_FRAGMENT_DTYPE.names == ("window", "bin", "hits", "n", "identity", "kept", "reserved")
    assert re.search(r"#define PG_K__END 23\b", text) and re.search(r"#define PG_K__COUNT 20\b", text)      # no new profiling slot


def test_unknown_mapping_is_refused_before_the_library_is_touched(tmp_path):
    from pyani_amd.engine import Engine
    from pyani_amd.multi import MultiEngine
    from pyani_amd.subcmd_fastani import run_fastani
    eng = Engine.__new__(Engine)      # no context, no library: the check comes first
    with pytest.raises(ValueError, match="nowhere"):
        eng.sketch_pairs([0], [0], mapping="nowhere")
    with pytest.raises(ValueError, match="nowhere"):
        MultiEngine.__new__(MultiEngine).sketch_pairs([0], [0], mapping="nowhere")
    with pytest.raises(ValueError, match="nowhere"):
        run_fastani(tmp_path, mapping="nowhere")
    with pytest.raises(ValueError):
        eng.sketch_pairs([0], [0], mapping=None)
