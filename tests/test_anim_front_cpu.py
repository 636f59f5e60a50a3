"""CPU: the directed front-end cases (tests/anim_front_cases.py) against the nucmer oracle and the host statement.

Every case, --mum and --maxmatch, A as the reference and B as the reference:
  * the oracle's records are exactly the case's claim (one record per claimed cluster, no other) — a case that does not sit
    on its threshold fails here, before any GPU sees it;
  * the statement (pg_anim_core.h through tools/anim_debug --dump --exact) gives the oracle's record set.
Where the two disagree the oracle decides: it is pinned on real MUMmer output (tests/test_nucmer_oracle.py)."""
import subprocess

import pytest

from tests import anim_front_cases as fc
from tests.conftest import ROOT


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    oracle = ROOT / "oracle" / "_build" / "nucmer_oracle"
    oracle.parent.mkdir(exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", str(ROOT / "oracle" / "nucmer_oracle.cpp"), "-o", str(oracle)], check=True)
    stmt = ROOT / "tools" / "anim_debug" / "anim_debug"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'pyani_amd' / 'csrc'}", str(stmt) + ".cpp", "-o", str(stmt)], check=True)
    cases = fc.all_cases()
    d = tmp_path_factory.mktemp("anim_front")
    paths = {c.name: fc.write_case(d, c) for c in cases}
    want = fc.oracle_records(oracle, paths)
    jobs = {}
    for (name, mm, sw) in want:
        pa, pb = paths[name][::-1] if sw else paths[name]
        jobs[(name, mm, sw)] = [stmt, pa, pb, "--dump", "--exact"] + (["--maxmatch"] if mm else [])
    return cases, want, fc.run_all(jobs)


def _report(bad):
    if bad:
        pytest.fail("\n".join([f"{len(bad)} (case, mode, direction) differ:"] + [f"  {k}" for k in list(bad)[:60]] +
                              [f"  {k}: {v}" for k, v in list(bad.items())[:6]]), pytrace=False)


def _legs():
    return [(mm, sw) for mm in (False, True) for sw in (False, True)]


def test_the_case_set_is_complete(world):
    cases, want, _ = world
    for fam, least in fc.FAMILY_MIN.items():
        assert sum(c.family == fam for c in cases) >= least, fc.FAMILIES[fam]
    for strand in (0, 1):      # every (reference start mod 32, query strand start mod 5), on either strand, in cases that claim records
        got = set()
        for c in cases:
            if c.family == 1 and c.expect[(False, False)] and c.planted[0].strand == strand:
                got |= fc.phase_classes(c)
        assert len(got) == fc.MASK_WORD * fc.SEED_STEP, strand
    assert fc.claimed_records(cases) >= fc.RECORD_FLOOR > 5000
    assert sum(len(v) for v in want.values()) == fc.claimed_records(cases)


@pytest.mark.parametrize("family", sorted(fc.FAMILIES))
def test_oracle_records_are_exactly_the_claim(world, family):
    cases, want, _ = world
    bad = {}
    for c in cases:
        for mm, sw in _legs():
            if c.family == family:
                p = fc.claim_problems(c, mm, sw, want[(c.name, mm, sw)])
                if p:
                    bad[(c.name, "maxmatch" if mm else "mum", "B vs A" if sw else "A vs B")] = p[:4]
    _report(bad)


@pytest.mark.parametrize("family", sorted(fc.FAMILIES))
def test_statement_gives_the_oracle_records(world, family):
    cases, want, stmt = world
    bad = {}
    for c in cases:
        for mm, sw in _legs():
            if c.family != family:
                continue
            r = stmt[(c.name, mm, sw)]
            assert r.returncode in (0, 4), (c.name, r.returncode, r.stderr[-200:])      # (4: no alignment at all)
            got, w = set(fc.parse_records(r.stdout)), set(want[(c.name, mm, sw)])
            if got != w:
                bad[(c.name, "maxmatch" if mm else "mum", "B vs A" if sw else "A vs B")] = {"missing": sorted(w - got)[:3], "surplus": sorted(got - w)[:3]}
    _report(bad)
