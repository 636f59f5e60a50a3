"""The directed fragments of tests/anib_frag_cases.py without a GPU: the yardstick the GPU test holds the fragment kernels to.

  claims   every case reaches the path it was built for, read from the host statement's trace (anib_cpu_pair_trace), and the trace
           changes no row;
  oracle   the rows parse_blast_tab uses equal those of the independent blastn oracle where the case is labelled "equal" and differ
           where it is labelled "differs: ..." (so a label cannot go stale); at least three quarters of the cases are equal;
  evalue   the smallest exact match that passes the e-value cut is the same in the host statement, in the oracle and in the closed
           formula of blast_stat.c evaluated in Python, for every (query length, database bases, records);
  power    variants of the host statement with ONE constant changed give other rows on some case of the group aimed at that constant:
           the comparison with the host statement would notice the corresponding error in a kernel;
  golden   the host statement's rows per case, as sha1 hashes (tests/golden/anib_frag_cases_sha1.txt): a change of the statement shows.
"""
import pytest

from tests import anib_frag_cases as cases

ALL = cases.all_cases()
IDS = [c.name for c in ALL]

# Each variant and the group aimed at it.  One constant the suite has NO power over: the refresh period of the shared best score.
# PGA_FRAG_XSYNC=1 (refreshed on every anti-diagonal; 8 and 16 likewise) was NOT OBSERVED to change a row: not of any directed case, not
# of 30 000 random fragments with gaps of 20 .. 85 bases in both directions (anib_frag_cases.zigzag_fragment over seeds 0 .. 23 999 and a
# free-running search), not of 400 tandem copies of 79 .. 84 bases whose second unit carries a substitution, with the locus at both
# parities.  A likely reason, not a proof: a state that only a stale best score keeps lies below a best score that is still RISING, and
# the alignment through it is also reached from the rising path by opening the gap later, where nothing depends on the refresh.  So a
# kernel that refreshed its copy at another period would pass this suite; the test below has no entry for it and says so here.
POWER = {"PGA_FRAG_XDROP=164": "gap", "PGA_FRAG_BAND=128": "edge", "PGA_FRAG_TRACK=32": "drift", "PGA_FRAG_SHIFT_MAX=6": "drift", "PGA_FRAG_SLACK=198": "slack",
         "PGA_FRAG_MIN_CLIP=12": "clip", "PGA_FRAG_WORD_FIRST=16": "seeds"}


def test_groups_and_sizes():
    assert {c.group for c in ALL} == set(cases.GROUPS) and len(ALL) >= 100
    for c in ALL:
        nfrag = sum(-(-int(b - a) // c.fragsize) for a, b in zip(c.query[1][:-1], c.query[1][1:]))
        assert nfrag <= 40 and (len(c.subject[0]) <= 62_000 or c.group == "evalue"), (c.name, nfrag, len(c.subject[0]))
    gap = {c.name for c in cases.by_group("gap")}
    assert gap >= {f"gap_{kind}_{k}" for kind in ("del", "ins") for k in cases.GAP_KS}
    assert len(cases.by_group("evalue")) == len(cases.EVALUE_QLEN) * len(cases.EVALUE_DB) * len(cases.EVALUE_NREC) == 24


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_claim_holds_on_the_trace_and_the_trace_changes_no_row(monkeypatch, case):
    t = cases.host_trace(case)
    assert t.rows == cases.host_pair(monkeypatch, case), case.name
    assert len(t.fs) % 2 == 0 and [int(x["frag"]) for x in t.fs[::2]] == list(range(len(t.fs) // 2))
    case.claim(t)      # an AssertionError here: the case does not reach its path


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_independent_oracle(case):
    label = cases.oracle_label(case)
    assert label == "equal" or (label.startswith("differs: ") and len(label) > 30), label
    same, rep = cases.used_equal(cases.host_trace(case).rows, case)
    assert same == (label == "equal"), (case.name, label, rep)


def test_three_quarters_of_the_cases_equal_the_oracle():
    equal = sum(cases.oracle_label(c) == "equal" for c in ALL)
    assert set(cases.ORACLE) <= set(IDS) and 4 * equal >= 3 * len(ALL), (equal, len(ALL))


def _mnN(case):
    return tuple(int(x[1:]) for x in case.name.split("_")[1:])


@pytest.mark.parametrize("case", cases.by_group("evalue"), ids=[c.name for c in cases.by_group("evalue")])
def test_evalue_threshold_host_oracle_formula(case):
    m, n, N = _mnN(case)
    host, host_mono = cases.lstar_of_rows(cases.host_trace(case).rows)
    orc, orc_mono = cases.lstar_of_rows(cases.rows_of(cases.oracle_rows(case)))
    formula = cases.formula_lstar(m, n, N)
    print(f"{case.name}: L* host {host}, oracle {orc}, formula {formula}")
    assert host_mono and orc_mono and host == orc == formula and cases.EVALUE_LS[0] < formula < cases.EVALUE_LS[-1], (host, orc, formula)


@pytest.mark.parametrize("define", sorted(POWER))
def test_a_changed_constant_changes_rows_of_its_group(monkeypatch, define):
    import oracle_build
    assert define in oracle_build.ANIB_CPU_VARIANTS
    changed = [c.name for c in cases.by_group(POWER[define]) if cases.host_pair(monkeypatch, c, defines=[define]) != cases.host_trace(c).rows]
    print(f"{define}: changes {len(changed)} of {len(cases.by_group(POWER[define]))} {POWER[define]} cases: {changed}")
    assert changed, define


def test_default_variant_is_the_statement(monkeypatch):
    # a variant built with the default value is the statement itself: the variants differ by their define and by nothing else
    for c in cases.by_group("edge") + cases.by_group("slack"):
        assert cases.host_pair(monkeypatch, c, defines=["PGA_FRAG_BAND=256"]) == cases.host_trace(c).rows, c.name


def test_golden_hashes():
    want = cases.GOLDEN.read_text()
    got = cases.golden_text()
    differing = [a.split()[0] for a, b in zip(got.splitlines(), want.splitlines()) if a != b]
    assert got == want, differing
