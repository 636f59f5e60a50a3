"""CPU-only: the case table of the trimmed searches (tests/search_cases.py) is what it claims to be, on the two CPU references alone.
pgn::ScalarEngine (the definition the wave engines follow) equals the independent restatement's align_engine (oracle/nucmer_oracle.cpp
--searches) on every search; the host emulation of the diagonal window equals the scalar engine wherever its window held the band; and
every group's claim holds — window moves in both directions, window misfits on 256 and on 512 diagonals, the three outcomes at the break
length, ties, the lane kernels' size classes and the proof they rest on.  tests/test_searches_gpu.py holds the GPU engines against the
same expectations."""
import pytest

from tests import search_cases as sc


@pytest.fixture(scope="module")
def table():
    return sc.cases(), sc.expected()


def _rows(table, group=None):
    cs, ex = table
    for c in cs:
        if group is None or c.group == group:
            for k, e in enumerate(ex[c.name]):
                yield c, k, e


def test_the_table_has_every_group_on_both_strands_and_in_every_mode(table):
    cs, ex = table
    assert {c.group for c in cs} == set(sc.GROUPS)
    for g in sc.GROUPS:
        mine = [c for c in cs if c.group == g]
        assert {c.strand for c in mine} == {0, 1}, g
        modes = {s[4] for c in mine for s in c.searches}
        assert modes == ({sc.FORWARD_ALIGN} if g == "lanes" else set(sc.MODES)), g
    assert sum(len(c.searches) for c in cs) >= 3000
    assert max(max(e["N"], e["M"]) for c, k, e in _rows(table)) == 10000


def test_scalar_engine_equals_the_independent_restatement(table):
    n = 0
    for c, k, e in _rows(table):
        assert e["scalar"] == e["oracle"], (c.name, k, c.searches[k])      # end, errors, reached
        n += 1
    assert n == sum(len(c.searches) for c in table[0])
    assert any(e["scalar"][2] > 1000 for c, k, e in _rows(table)) and any(e["scalar"][3] == 0 for c, k, e in _rows(table))


def test_emulated_windows_equal_the_scalar_engine_wherever_they_fit(table):
    fits = {4: 0, 8: 0}
    for c, k, e in _rows(table):
        for dpl in (4, 8):
            w = e[f"e{dpl}"]
            if w["fit"]:
                assert (w["result"], w["score"], w["wmax"]) == (e["scalar"], e["score"], e["wmax"]), (c.name, k, dpl)
                fits[dpl] += 1
            else:
                assert w["result"] == (0, 0, 0, 0)
        assert e["e8"]["fit"] or not e["e4"]["fit"], (c.name, k)      # what 512 diagonals cannot hold, 256 cannot either
    assert fits[8] > fits[4] > 3000


def test_drift_cases_move_the_window_both_ways(table):
    seen = set()
    for c, k, e in _rows(table, "drift"):
        w4, w8 = e["e4"], e["e8"]
        assert w4["fit"] and w8["fit"] and w4["moves"] > 0 and w4["moves"] == w4["down"] + w4["up"], (c.name, k)
        if c.what == "two-way":
            assert w4["down"] > 0 and w4["up"] > 0, (c.name, k, w4)
        else:
            assert (w4["down"] > 0) != (w4["up"] > 0), (c.name, k, w4)
            seen.add(("down" if w4["down"] else "up", e["m_o"]))
        assert e["scalar"][2] > 100      # (the path was followed: hundreds of gap bases)
    assert seen == {(d, m) for d in ("down", "up") for m in sc.MODES}
    assert any(e["e8"]["moves"] > 0 for c, k, e in _rows(table, "drift"))


def test_outgrow_cases_do_not_fit_the_window_they_claim(table):
    held_by = set()
    for c, k, e in _rows(table, "outgrow"):
        assert e["e4"]["fit"] == 0, (c.name, k)
        assert e["e8"]["fit"] == (1 if c.what == 512 else 0), (c.name, k, e["wmax"])
        assert e["wmax"] > 125 and (c.what == 512 or e["wmax"] > 253)      # cells per anti-diagonal: two diagonals apart
        held_by.add((c.what, e["m_o"], c.strand))
    assert held_by == {(w, m, s) for w in (512, 0) for m in sc.MODES for s in (0, 1)}
    # nothing else in the table outgrows a window: the misfits of the GPU tests are these cases'
    assert all(e["e4"]["fit"] for c, k, e in _rows(table) if c.group != "outgrow")
    # ... and the largest of them stays within what the global-engine test runs directly
    assert max(max(e["N"], e["M"]) for c, k, e in _rows(table, "outgrow")) <= 3000


def test_break_cases_sit_on_the_break_length(table):
    cs, ex = table
    got = {}
    for c in cs:
        if c.group != "break":
            continue
        for k, e in enumerate(ex[c.name]):
            end = (sc.BREAK_GOOD - 1,) * 2 if c.name.split("_")[2] == "fwd" else (len(c.a) - sc.BREAK_GOOD, len(c.b if not c.strand else c.b) - sc.BREAK_GOOD)
            if e["m_o"] & sc.OPTIMAL_BIT or not e["scalar"][3]:      # the best cell: the end of the good stretch, nothing after it ties
                assert e["scalar"][:2] == end and e["scalar"][2] == 0 and e["score"] == 3 * sc.BREAK_GOOD and e["ties"] == 1, (c.name, k)
            got[(c.what, c.name.split("_")[2], c.strand, e["m_o"])] = e["scalar"][3]
            assert e["N"] + e["M"] == 2 * sc.BREAK_GOOD + c.what
    for d, modes in (("fwd", sc.FWD_MODES), ("bwd", sc.BWD_MODES)):
        for s in (0, 1):
            # to the target: reached while the matrix ends within BREAK_LEN anti-diagonals of the last best cell, not one later
            assert [got[(t, d, s, modes[0])] for t in (199, 200, 201)] == [1, 1, 0], (d, s)
            assert [got[(t, d, s, modes[1])] for t in (199, 200, 201)] == [0, 0, 0], (d, s)      # best cell: it is not the corner


def test_ties_cases_have_ties(table):
    """What `ties` can claim.  A repeat against itself (or against one copy more) has ONE best cell, the end of the shorter side: no gap
    of a homopolymer or tandem pays for itself (3 k = 10 + 7 g only at g = 3, k = 8).  What such a case does have is anti-diagonal after
    anti-diagonal whose best score is shared by two or more cells, and cells whose three states tie: the restatement counts those
    anti-diagonals.  The two designed cases then put the tie on the FINAL best score, where the rule decides the finish."""
    cs, ex = table
    for c, k, e in _rows(table, "ties"):
        if c.what is None:
            assert e["tied_diagonals"] >= min(e["N"], e["M"]) // 2 - 1 > 20, (c.name, k, e["tied_diagonals"])
        else:
            assert e["ties"] >= 2, (c.name, k, e["ties"])
    for c in cs:
        if c.what == "same":       # the larger j wins on one anti-diagonal: the finish lies 8 rows / 11 columns past the prefix
            e = next(e for e in ex[c.name] if e["m_o"] & sc.OPTIMAL_BIT)
            p = len(c.a) - 11
            fin = (p + 7, p + 10) if "_fwd_" in c.name else (len(c.a) - 1 - (p + 7), len(c.a) - 1 - (p + 10))
            assert e["scalar"][:2] == fin and e["score"] == 3 * p and e["ties"] == 3, (c.name, e)
        if c.what == "later":      # `>=` moves the finish forward: the corner, and a best-cell search says reached
            e = next(e for e in ex[c.name] if e["m_o"] & sc.OPTIMAL_BIT)
            corner = (len(c.a) - 1, len(c.a) - 4) if "_fwd_" in c.name else (0, 0)
            assert e["scalar"][:2] == corner and e["scalar"][3] == 1 and e["ties"] == 2 and e["scalar"][2] == 3, (c.name, e)


def test_ends_and_residues_are_where_the_table_says(table):
    cs, ex = table
    for c in cs:
        if c.group == "ends":
            la, lb = len(c.a), len(c.b)
            starts = {(s[0], s[1]) for s in c.searches}
            targets = {(s[2], s[3]) for s in c.searches}
            for d in sc.END_DISTANCES:
                assert {(d, d), (la - 1 - d, lb - 1 - d)} <= starts and {(la - 1 - d, lb - 1 - d), (d, d)} <= targets | starts
            assert any(s[0] < 32 and s[4] == sc.BACKWARD_SEARCH for s in c.searches)                       # backwards from below position 32
            assert any(s[2] == la - 1 and s[3] == lb - 1 and s[4] == sc.FORWARD_ALIGN for s in c.searches)      # forwards into the last base
            assert any(ex[c.name][k]["N"] == 1 and ex[c.name][k]["M"] > 80 for k in range(len(c.searches)))
            assert any(ex[c.name][k]["M"] == 1 and ex[c.name][k]["N"] > 80 for k in range(len(c.searches)))
        if c.group == "residues":
            col = 0 if "_A0_" in c.name else 1
            assert {s[col] % 32 for s in c.searches if s[4] & 1} == set(range(32))
            assert {s[col] % 32 for s in c.searches if not s[4] & 1} == set(range(32))


def test_unclean_cases_hold_what_they_claim(table):
    cs, ex = table
    by = {c.name: c for c in cs}
    bs = lambda c: sc.revcomp(c.b) if c.strand else c.b      # noqa: E731  (the strand the B coordinates index)
    for s in (0, 1):
        assert by[f"unclean_start_base_s{s}"].a[0] == "N" and bs(by[f"unclean_start_base_b_s{s}"])[0] == "N"
        assert by[f"unclean_target_base_s{s}"].a[-1] == "N" and bs(by[f"unclean_target_base_b_s{s}"])[-1] == "N"
        assert "N" * 40 in by[f"unclean_run_40_in_b_s{s}"].b and "N" * 40 in by[f"unclean_run_40_in_a_s{s}"].a
        assert by[f"unclean_every_97_s{s}"].b.count("N") >= 14
        base = None
        for d in (301, 280, 150, 20):
            c = by[f"unclean_outside_{d}_s{s}"]
            (a0, b0, a1, b1), = c.rects
            assert c.a.count("N") == 1 and c.b.count("N") == 1 and c.a.index("N") == a0 - d and bs(c).index("N") == b1 + d
            res = [(e["scalar"], e["score"]) for e in ex[c.name]]      # an unclean base outside the matrix changes nothing
            base = base or res
            assert res == base and any(e["scalar"][2] > 0 for e in ex[c.name])


def test_lane_rectangles_cannot_be_trimmed_and_cannot_break(table):
    """The proof the one-gap-per-lane kernels rest on, tested: on a rectangle with both sides <= 59 MUMmer's trimmed, breakable search
    reaches its target, and its error count is that of the plain untrimmed global alignment (plain integers: forced_referee.h)."""
    shapes, per_class, n_big = set(), {}, 0
    for c, k, e in _rows(table, "lanes"):
        cls = sc.lane_class(e["N"], e["M"])
        if cls is None:
            n_big += 1
            assert e["global_errors"] == -1 and {e["N"], e["M"]} == {60, 10}
            continue
        assert e["scalar"][3] == 1 and e["scalar"][:2] == c.searches[k][2:4], (c.name, k)      # target reached
        assert e["global_errors"] == e["scalar"][2], (c.name, k, e["N"], e["M"])
        shapes.add((e["N"], e["M"]))
        per_class[cls] = per_class.get(cls, 0) + 1
    assert shapes >= {(n, m) for n in sc.LANE_SIDES for m in sc.LANE_SIDES} and n_big >= 20 and set(per_class) == set(sc.LANE_CLASSES)
    cs, ex = table
    for c in cs:
        if c.name.startswith("lanes_list_"):      # 64 k + 1 gaps, all of one class: the last wave has one live lane
            assert len(c.searches) % 64 == 1 and {sc.lane_class(e["N"], e["M"]) for e in ex[c.name]} == {c.what}, c.name
    assert {len(c.searches) for c in cs if c.name.startswith("lanes_list_")} == {1, 129}
    ident = {c.name: sum(e["scalar"][2] for e in ex[c.name] if e["N"] == e["M"]) for c in cs if c.name.startswith("lanes_identity_")}
    for s in (0, 1):      # identity from 100 % down to unrelated, on the squares (elsewhere the sides' difference counts too): errors grow from none
        errs = [ident[f"lanes_identity_{i}_s{s}"] for i in sc.LANE_IDENTITIES]
        assert errs[0] == 0 and errs == sorted(errs) and errs[-1] > 4 * errs[1] > 0, errs
    # every comparison above is on rectangles no larger than 59: also every OTHER forward search of that size in the table agrees
    for c, k, e in _rows(table):
        if e["global_errors"] >= 0 and e["m_o"] == sc.FORWARD_ALIGN:
            assert e["global_errors"] == e["scalar"][2] and e["scalar"][3] == 1, (c.name, k)


def test_the_list_call_holds_every_search_once():
    by_name = {c.name: c for c in sc.cases()}
    for lanes in (False, True):
        total = 0
        for strand in (0, 1):
            a, b, searches, who = sc.list_call(strand, lanes)
            bs = sc.revcomp(b) if strand else b
            assert len(searches) == len(set(who)) >= 300
            for (A0, B0, tA, tB, m_o), (name, k, a_off, b_off) in zip(searches, who):
                c = by_name[name]
                a0, b0, ta, tb, m = c.searches[k]
                cb = sc.revcomp(c.b) if strand else c.b
                lo, hi = (A0, tA) if m & 1 else (tA, A0)
                l2, h2 = (a0, ta) if m & 1 else (ta, a0)
                assert m == m_o and a[lo:hi + 1] == c.a[l2:h2 + 1] and (A0 - a0, B0 - b0) == (a_off, b_off), (name, k)
                lo, hi = (B0, tB) if m & 1 else (tB, B0)
                l2, h2 = (b0, tb) if m & 1 else (tb, b0)
                assert bs[lo:hi + 1] == cb[l2:h2 + 1], (name, k)
            total += len(searches)
        assert total >= (1000 if lanes else 3000)
