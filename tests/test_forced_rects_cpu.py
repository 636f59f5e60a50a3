"""CPU-only: the case table of the forced re-alignment ladder (tests/forced_cases.py) is what it claims to be.  For every rectangle
the plain-integer referee, pgn::ScalarEngine and pgd::DiagWaveEngine agree (tools/anim_debug/forced_rects.cpp runs all three), the
logged ladder of bands is the one the table claims, and the table as a whole reaches every kernel class and both sides of every
window threshold.  tests/test_forced_rects_gpu.py holds the GPU kernels against the same expectations."""
import pytest

from tests import forced_cases as fc


@pytest.fixture(scope="module")
def table():
    return fc.cases(), fc.expected()


def _rows(table):
    cs, ex = table
    for c in cs:
        for k, e in enumerate(ex[c.name]):
            yield c, k, e


def test_restated_thresholds_are_the_window_rule():
    """62 DPL + 2 diagonals are sure to fit a window of 64 DPL; the group of four waves takes 256 DPL - 8."""
    assert fc.THR_NARROW == tuple(62 * d + 2 for d in fc.DPL_NARROW)
    assert fc.THR_WIDE == tuple(62 * d + 2 for d in fc.DPL_WIDE)
    assert fc.THR_GROUP == tuple(256 * d - 8 for d in fc.DPL_GROUP)
    assert fc.span_of(100, 164, 28) == 126 and fc.span_of(164, 100, 28) == 126 and fc.span_of(28, 1, -1) == 35


def test_referee_scalar_engine_and_wave_emulation_agree(table):
    n = 0
    for c, k, e in _rows(table):
        where = (c.name, k)
        assert e["loops_ok"], where                       # the engines' own align() is the logged loop
        assert (e["diag_status"], e["diag_errors"], e["diag_ladder"]) == (e["status"], e["errors"], e["ladder"]), where
        if e["status"] == 0:
            assert e["errors"] == e["ref_errors"], where
        else:      # the verdict: the engines give up exactly where the plain-integer optimal path leaves the score field
            assert e["status"] == 2 and e["errors"] == 0 and e["ref_min"] < fc.FLOOR and e["ladder"][-1] == -1, where
        n += 1
    assert n == sum(len(c.rects) for c in table[0]) >= 300


def test_every_ladder_is_the_one_the_table_claims(table):
    for c, k, e in _rows(table):
        got = fc.dispatch(e["spans"])
        if c.claim is not None:
            assert tuple(kern for kern, _ in got) == c.claim[k], (c.name, k, e["ladder"], e["spans"])
        if c.first is not None:
            assert (e["spans"][0],) + got[0] == c.first and e["ladder"][0] == fc.FIRST_BAND, (c.name, e["spans"])
        assert e["ladder"][0] == (fc.FIRST_BAND if max(e["N"], e["M"]) > fc.FIRST_BAND else -1)
        assert all(w == -1 or w % 4 == 0 for w in e["ladder"][1:]) and e["w_used"] == (0 if e["status"] else e["ladder"][-1])


def test_boundary_cases_sit_on_both_sides_of_every_threshold(table):
    cs, ex = table
    seen = {}
    for c in cs:
        if c.group != "boundary":
            continue
        e = ex[c.name][0]
        assert c.first is not None
        span, kern, dpl = c.first
        info = seen.setdefault(span, dict(kern=kern, dpl=dpl, orient=set(), pos=set(), certified=False))
        info["orient"].add(e["N"] > e["M"])
        info["pos"].add(c.name.split("_")[2])
        info["certified"] |= e["status"] == 0 and len(e["ladder"]) == 1 and e["errors"] == span - 62 > 0
    for T in fc.ALL_THRESHOLDS:
        assert T in seen and T + 1 in seen, T
        # the two sides are taken by different engines (or kernels): that is what makes T a boundary
        assert (seen[T]["kern"], seen[T]["dpl"]) != (seen[T + 1]["kern"], seen[T + 1]["dpl"]), T
        if T <= 3064:      # (beyond span 3331 no rectangle of at most 10 000 bases a side certifies at the first band: see the table's text)
            assert seen[T]["certified"] and seen[T + 1]["certified"], T
    assert seen[8185]["kern"] == "strips" and seen[8184] == dict(seen[8184], kern="group", dpl=32)
    assert {o for i in seen.values() for o in i["orient"]} == {True, False}
    assert {p for i in seen.values() for p in i["pos"]} == {"start", "middle", "end"}
    narrow_wide = [i for s, i in seen.items() if s < 1490]
    assert all(i["orient"] == {True, False} for i in narrow_wide)


def test_every_kernel_class_engine_and_hand_over_is_reached(table):
    engines, handovers, whole_ok, certified_in = set(), set(), 0, set()
    for c, k, e in _rows(table):
        got = fc.dispatch(e["spans"])
        engines.update(got)
        handovers.update((a[0], b[0]) for a, b in zip(got, got[1:]) if a[0] != b[0])
        whole_ok += e["status"] == 0 and e["ladder"][-1] == -1
        if e["status"] == 0 and e["errors"] > 0:
            certified_in.add(got[-1])
    want = {("narrow", d) for d in fc.DPL_NARROW} | {("wide", d) for d in fc.DPL_WIDE[1:]} | {("group", d) for d in fc.DPL_GROUP} | {("strips", 0)}
    assert engines == want      # (the wide kernel's 512-diagonal window belongs to the knob configurations: the narrow kernel has it too)
    assert {("narrow", "wide"), ("wide", "group"), ("group", "strips")} <= handovers
    assert whole_ok >= 20
    # a certified, non-zero error count comes out of every single-wave window and of the group's 3072 / 4096 forms; the group's
    # wider forms and the strips see only unreachable corners in the default configuration (the knob runs put certified runs there)
    assert certified_in >= want - {("group", 24), ("group", 32), ("strips", 0)}


def test_every_group_has_errors_and_the_table_is_not_trivial(table):
    by_group = {g: [] for g in fc.GROUPS}
    for c, k, e in _rows(table):
        if c.group != "limits":
            by_group[c.group].append(e)
    for g, es in by_group.items():
        assert es and any(e["status"] == 0 and e["errors"] > 0 for e in es), g
    assert sum(e["status"] == 2 for e in by_group["floor"]) == 1 and by_group["floor"][1]["status"] == 2
    assert by_group["floor"][0]["ref_min"] < -1100 and by_group["floor"][0]["status"] == 0      # case A: a deep dip, exact
    tiny = {(e["N"], e["M"]) for e in by_group["tiny"]}
    assert tiny == {(n, m) for n in (1, 2, 27, 28, 29) for m in (1, 2, 27, 28, 29)}


def test_tie_cases_depend_on_the_tie_order(table):
    """Homopolymers and repeats have many optimal paths, but a rectangle tells a wrong tie order from the right one only if the orders
    COUNT differently on it.  The referee under DELETE > INSERT > MATCH differs from MUMmer's MATCH > INSERT > DELETE on every
    'sensitive' case — both strands, windows of 256 and 384 diagonals.  (Swapping INSERT and DELETE alone — the referee's order 1 — changed no count on
    49 000 random low-complexity rectangles searched for this table, so no case can be offered for that swap.)"""
    cs, ex = table
    sens = [c for c in cs if c.name.startswith("ties_sensitive_")]
    assert len(sens) >= 8 and {c.strand for c in sens} == {0, 1}
    dpls = set()
    for c in sens:
        e = ex[c.name][0]
        assert e["status"] == 0 and e["errors"] == e["ref_errors"] and len(e["ladder"]) == 1, c.name
        assert e["alt_errors"][1] not in (-1, e["ref_errors"]), (c.name, e["alt_errors"])
        dpls.add(fc.dispatch(e["spans"])[0])
    assert dpls == {("narrow", 4), ("narrow", 6)}      # beyond the 128-diagonal window
    for c, k, e in _rows(table):      # (the other orders are counted wherever the rectangle has at most a million cells)
        assert (e["alt_errors"][0] == -1) == (e["N"] * e["M"] > 1 << 20), (c.name, k)


def test_the_list_call_holds_every_rectangle_once():
    total = 0
    for strand in (0, 1):
        a, b, rects, who = fc.list_call(strand)
        by_name = {c.name: c for c in fc.cases()}
        bs = fc.revcomp(b) if strand else b
        assert len(rects) == len(set(who)) >= 100
        for (A0, A1, B0, B1), (name, k) in zip(rects, who):
            c = by_name[name]
            a0, a1, b0, b1 = c.rects[k]
            cb = fc.revcomp(c.b) if strand else c.b
            assert a[A0:A1 + 1] == c.a[a0:a1 + 1] and bs[B0:B1 + 1] == cb[b0:b1 + 1], (name, k)
        short = sum((A1 - A0) + (B1 - B0) <= 1500 for A0, A1, B0, B1 in rects)
        assert 0 < short < len(rects)      # both request lists
        total += len(rects)
    assert total >= 300
