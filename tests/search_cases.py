"""Directed TRIMMED searches for the search engines of the ANIm extender (pga_postnuc.inc / pga_postnuc_diag.inc: the 256- and the
512-diagonal window, the global-memory engine and the one-gap-per-lane kernels behind pg_anim_searches), with what is expected of
each: the result of pgn::ScalarEngine::run (the definition the wave engines follow), what the host emulation of the diagonal window
did on 256 and on 512 diagonals (fit, window moves and their direction; tools/anim_debug/searches.cpp), the answer of the independent
restatement (oracle/nucmer_oracle.cpp --searches: its own align_engine, which reproduces every MUMmer fixture file and shares nothing
with the product) with the number of cells that held the final best score, and for the lane kernels' rectangles the error count of
the plain untrimmed global alignment.

A search is (A0, B0, tA, tB, m_o): start and target as stream positions, B in the coordinates of the query strand; m_o one of
FORWARD_ALIGN (1), FORWARD_ALIGN | OPTIMAL_BIT (9), BACKWARD_SEARCH (2), BACKWARD_SEARCH | OPTIMAL_BIT (10).  A case's `rects` are
corner pairs (a0, b0, a1, b1), a0 <= a1, b0 <= b1: forward modes search from (a0, b0) towards (a1, b1), backward ones from (a1, b1)
towards (a0, b0).  Sequences come from seeded generators; the `outgrow` cases are constructed too, after a harvest over the project's
synthetic workloads (tools/anim_debug/harvest_searches.py) turned up no search at all that the 256-diagonal window does not hold.

The engine's numbers restated here: +3 a match, -7 a mismatch or a gap's further base, -10 a gap's first base; a band cell more than
600 below the best score is trimmed; a search ends 200 anti-diagonals after its last best cell (a tie moves the finish forward:
`>=`, and on one anti-diagonal the larger j wins).
"""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

FORWARD_ALIGN, BACKWARD_SEARCH, OPTIMAL_BIT = 1, 2, 8
MODES = (FORWARD_ALIGN, FORWARD_ALIGN | OPTIMAL_BIT, BACKWARD_SEARCH, BACKWARD_SEARCH | OPTIMAL_BIT)
FWD_MODES, BWD_MODES = MODES[:2], MODES[2:]
BREAK_LEN = 200
PN_SMALL = 59                                   # the lane kernels take gaps with both sides up to this ...
LANE_CLASSES = (16, 32, PN_SMALL)               # ... by the larger side
LANE_SIDES = (1, 2, 15, 16, 17, 31, 32, 33, 58, 59)
GROUPS = ("plain", "break", "ties", "drift", "ends", "residues", "unclean", "outgrow", "lanes")

_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def other_base(rng, c):
    return "ACGT"[("ACGT".index(c) + 1 + int(rng.integers(0, 3))) & 3]


def substitute(rng, s, positions):
    t = list(s)
    for p in positions:
        t[p] = other_base(rng, t[p])
    return "".join(t)


def mutate(rng, a, sub, indel, n_every=0):
    """tools/anim_debug/norm_check.cpp's mutate: substitutions at rate sub and single-base insertions / deletions at rate indel (per
    mille), an N every n_every bases."""
    out = []
    for i, c in enumerate(a):
        if int(rng.integers(0, 1000)) < indel:
            if int(rng.integers(0, 2)):
                continue
            out.append("ACGT"[int(rng.integers(0, 4))])
        if int(rng.integers(0, 1000)) < sub:
            c = other_base(rng, c)
        if n_every and i % n_every == n_every - 1:
            c = "N"
        out.append(c)
    return "".join(out)


class Case:
    """name, group, reference, query AS STORED (the forward strand), strand, searches (A0, B0, tA, tB, m_o).  lanes: the case runs
    through the LANES engine too (all its searches are FORWARD_ALIGN).  what: the group's claim this case carries (the CPU test reads it)."""

    def __init__(self, name, group, a, b_strand, strand, rects, modes=MODES, lanes=False, what=None):
        self.name, self.group, self.a, self.strand, self.lanes, self.what = name, group, a, strand, lanes, what
        self.b = revcomp(b_strand) if strand else b_strand      # (b_strand: what the searches' B coordinates index)
        self.rects = [tuple(int(v) for v in r) for r in (rects if rects is not None else [(0, 0, len(a) - 1, len(b_strand) - 1)])]
        self.modes = tuple(modes)
        self.searches = []
        for a0, b0, a1, b1 in self.rects:
            assert 0 <= a0 <= a1 < len(a) and 0 <= b0 <= b1 < len(b_strand), (name, a0, b0, a1, b1)
            for m in self.modes:
                self.searches.append((a0, b0, a1, b1, m) if m & 1 else (a1, b1, a0, b0, m))

    def sides(self, k):
        A0, B0, tA, tB, _ = self.searches[k]
        return abs(tA - A0) + 1, abs(tB - B0) + 1


def _both(name, group, a, b, rects=None, **kw):
    return [Case(f"{name}_s{s}", group, a, b, s, rects, **kw) for s in (0, 1)]


def _directed(name, group, a, b, rects=None, **kw):
    """A case whose point lies in the direction of the walk: forwards as built, and backwards on the mirrored sequences."""
    out = []
    for s in (0, 1):
        out.append(Case(f"{name}_fwd_s{s}", group, a, b, s, rects, modes=FWD_MODES, **kw))
        out.append(Case(f"{name}_bwd_s{s}", group, a[::-1], b[::-1], s, None if rects is None else
                        [(len(a) - 1 - a1, len(b) - 1 - b1, len(a) - 1 - a0, len(b) - 1 - b0) for a0, b0, a1, b1 in rects], modes=BWD_MODES, **kw))
    return out


# ---- plain: the cases of tools/anim_debug/norm_check.cpp ---------------------------------------------------------------------------
def _plain_cases():
    out = []
    rng = np.random.default_rng(6101)
    a = rand_seq(rng, 10000)      # 30 matching bases, 16 substituted ones: the search just keeps finding a new best cell
    out += _both("plain_long_low", "plain", a, substitute(rng, a, [i for i in range(len(a)) if i % 46 >= 30]))
    rng = np.random.default_rng(6102)
    a = rand_seq(rng, 10000)
    out += _both("plain_long_exact", "plain", a, a)
    rng = np.random.default_rng(6103)
    a = rand_seq(rng, 6000)
    out += _both("plain_indels", "plain", a, mutate(rng, a, 20, 25))
    rng = np.random.default_rng(6104)
    out += _both("plain_unrelated", "plain", rand_seq(rng, 3000), rand_seq(rng, 3000))
    rng = np.random.default_rng(6105)
    a = rand_seq(rng, 4000)
    out += _both("plain_tail_drop", "plain", a, mutate(rng, a[:2000], 30, 3) + rand_seq(rng, 2000))
    rng = np.random.default_rng(6106)
    a = rand_seq(rng, 5000)
    out += _both("plain_with_N", "plain", a, mutate(rng, a, 40, 2, 97))
    rng = np.random.default_rng(6107)
    out += _both("plain_strip_1x400", "plain", rand_seq(rng, 1), rand_seq(rng, 400))
    rng = np.random.default_rng(6108)
    a = rand_seq(rng, 12)
    b = substitute(rng, a, [4, 9])
    out += _both("plain_tiny", "plain", a, b, [(o, o, o + n - 1, o + m - 1) for n in range(1, 7) for m in range(1, 7) for o in (0, 3, 6)])
    return out


# ---- break: the matrix ends 199, 200, 201 anti-diagonals after the last best cell --------------------------------------------------
BREAK_GOOD = 300


def _break_pair(t):
    """BREAK_GOOD equal bases (the only best cell: their end, anti-diagonal 2 * BREAK_GOOD), then tails of t bases in all whose columns
    are mismatch, match, match, ...: every prefix sums below zero (no new best, no tie), and 100 columns lose ~35 points, so
    the band is never trimmed away (all-mismatch tails would lose 700 and be trimmed before the break length is reached).  N + M = 2 * BREAK_GOOD + t."""
    rng = np.random.default_rng(6200 + t)
    good = rand_seq(rng, BREAK_GOOD)
    tb = t // 2
    tail = rand_seq(rng, t - tb)
    return good + tail, good + substitute(rng, tail[:tb], range(0, tb, 3))


def _break_cases():
    out = []
    for t in (BREAK_LEN - 1, BREAK_LEN, BREAK_LEN + 1):
        a, b = _break_pair(t)
        out += _directed(f"break_{t}", "break", a, b, what=t)
    return out


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def _ties_cases():
    out = []
    rng = np.random.default_rng(6300)
    units = {"homopolymer": "A", "tandem2": "AC", "tandem7": rand_seq(rng, 7), "tandem8": rand_seq(rng, 8)}
    assert len(set(units["tandem7"])) > 1 and len(set(units["tandem8"])) > 1
    for name, u in units.items():
        k = 64 // len(u) + 1
        out += _both(f"ties_{name}_self", "ties", u * k, u * k)
        out += _both(f"ties_{name}_a_longer", "ties", u * (k + 1), u * k)
        out += _both(f"ties_{name}_b_longer", "ties", u * k, u * (k + 1))
    # Equal best scores on ONE anti-diagonal: after the common prefix P (score 3 |P| at its end) a's tail CCCGGGCCCGG and b's tail
    # GGGCCCGGGCC mismatch in every column, but skipping three bases of either (-10 -7 -7) is followed by eight matches (+24): the cells
    # (|P| + 11, |P| + 8) and (|P| + 8, |P| + 11) hold the best score again, on the same anti-diagonal -> the larger j is the finish.
    rng = np.random.default_rng(6301)
    P = rand_seq(rng, 40)[:-1] + "T"
    out += _directed("ties_one_antidiagonal", "ties", P + "CCCGGGCCCGG", P + "GGGCCCGGGCC", what="same")
    # ... on a LATER anti-diagonal: a = P + CCC + Q, b = P + Q with eight bases Q: the corner (|P| + 11, |P| + 8) ties the end of P
    # (`>=`: the finish moves forward, and a best-cell search reports the corner reached)
    Q = "GTAGTGAT"
    out += _directed("ties_later_antidiagonal", "ties", P + "CCC" + Q, P + Q, what="later")
    return out


# ---- drift: the window has to move -------------------------------------------------------------------------------------------------
def _drop_every(s, k):
    return "".join(c for i, c in enumerate(s) if i % k != k - 1)


def _drift_cases():
    out = []
    rng = np.random.default_rng(6400)
    a = rand_seq(rng, 8000)
    out += _both("drift_deletions", "drift", a, _drop_every(a, 25), what="one-way")        # 320 diagonals one way
    out += _both("drift_insertions", "drift", _drop_every(a, 25), a, what="one-way")       # ... and the other
    rng = np.random.default_rng(6401)
    a = rand_seq(rng, 8000)
    out += _both("drift_there_and_back", "drift", _drop_every(a[:4000], 25) + a[4000:], a[:4000] + _drop_every(a[4000:], 25), what="two-way")
    return out


# ---- ends: starts and targets within 0 ... 33 bases of the streams' ends -----------------------------------------------------------
END_DISTANCES = (0, 1, 2, 15, 16, 17, 30, 31, 32, 33)


def _ends_cases():
    out = []
    rng = np.random.default_rng(6500)
    a = rand_seq(rng, 173)
    b = mutate(rng, a, 60, 10)
    la, lb = len(a), len(b)
    rects = []
    for d in END_DISTANCES:
        rects += [(d, d, la - 1, lb - 1), (0, 0, la - 1 - d, lb - 1 - d), (0, 0, d, d + 1), (la - 1 - d, lb - 2 - d, la - 1, lb - 1),
                  (d, 0, la - 1, lb - 1 - d), (0, d, la - 1 - d, lb - 1)]
    rects += [(0, 0, 0, lb - 1), (la - 1, 0, la - 1, lb - 1), (40, 3, 40, 90), (0, 0, la - 1, 0), (0, lb - 1, la - 1, lb - 1), (5, 50, 120, 50)]      # strips: N = 1, M = 1
    out += _both("ends", "ends", a, b, rects)
    return out


# ---- residues: A0 mod 32 and B0 mod 32 ---------------------------------------------------------------------------------------------
def _residues_cases():
    out = []
    for which in ("A", "B"):
        rng = np.random.default_rng(6600 + (which == "B"))
        a, b, rects = list(rand_seq(rng, 96 * 33)), list(rand_seq(rng, 96 * 33)), []
        for r in range(32):
            core = rand_seq(rng, 60)
            mut = (mutate(rng, core, 80, 15) + rand_seq(rng, 4))[:60]      # (60 bases too: the backward searches' starts run through the residues as well)
            pa, pb = (96 * r + r, 96 * r + 7) if which == "A" else (96 * r + 7, 96 * r + r)
            a[pa:pa + len(core)] = core
            b[pb:pb + len(mut)] = mut
            rects.append((pa, pb, pa + len(core) - 1, pb + len(mut) - 1))
        assert len(a) == len(b) == 96 * 33 and {(r[0] if which == "A" else r[1]) % 32 for r in rects} == set(range(32))
        out += _both(f"residues_{which}0", "residues", "".join(a), "".join(b), rects)
    return out


# ---- unclean: bases that are not A, C, G, T ----------------------------------------------------------------------------------------
def _unclean_cases():
    out = []
    rng = np.random.default_rng(6700)
    a = rand_seq(rng, 1500)
    out += _both("unclean_every_97", "unclean", a, mutate(rng, a, 30, 3, 97))
    rng = np.random.default_rng(6701)
    a = rand_seq(rng, 600)
    b = mutate(rng, a, 30, 0)
    out += _both("unclean_run_40_in_b", "unclean", a, b[:280] + "N" * 40 + b[320:])
    out += _both("unclean_run_40_in_a", "unclean", a[:250] + "N" * 40 + a[290:], b)
    out += _both("unclean_start_base", "unclean", "N" + a[1:], b)
    out += _both("unclean_start_base_b", "unclean", a, "N" + b[1:])
    out += _both("unclean_target_base", "unclean", a[:-1] + "N", b)
    out += _both("unclean_target_base_b", "unclean", a, b[:-1] + "N")
    # the clean / not-clean form of a refill is chosen WAVE-wide, by windows that reach up to 160 (256 diagonals) / 288 (512) bases beyond the
    # band: a search of 100 bases with no unclean base within 300 bases of it and one just outside; then the same with that base inside the reach
    rng = np.random.default_rng(6702)
    a = rand_seq(rng, 1000)
    b = mutate(rng, a, 50, 0)
    for d in (301, 280, 150, 20):
        an = a[:450 - d] + "N" + a[451 - d:]
        bn = b[:549 + d] + "N" + b[550 + d:]
        out += _both(f"unclean_outside_{d}", "unclean", an, bn, [(450, 450, 549, 549)])
    return out


# ---- outgrow: searches whose band the 256-diagonal window (and for two of them the 512-diagonal one) does not hold -----------------
# HARVEST.  tools/anim_debug/harvest_searches.py ran the host statement with the emulated wave engines and its fallback log (extended by
# the call's positions) over the synthetic workloads the project generates: pairs of C4's families 0 - 3 (8 at 1 Mb, 22 at the full 5 Mb)
# and 7 pairs of C3's family 3 (at 1 Mb and at 5 Mb), 24 rearranged, 40 tandem and 44 two-strand stress pairs of tests/stress_genomes.py, and the five tandem
# genome pairs of tests/test_seed_passes_gpu.py: 983 910 calls of the 256-diagonal engine looked at, NONE of which its window did not
# hold (the archived counters of whole C4 grids say the same: 24 million calls, `overflows 0`).  So nothing could be cut out of a workload.
# CONSTRUCTION instead.  The band is an interval that is trimmed only from its EDGES, so two equally good paths that move apart keep
# everything between them alive.  Block t of the reference is (U V) repeated, of the query (V U) repeated, |U| = |V| = d (U, V
# unrelated): the diagonals +d and -d match perfectly, diagonal 0 not at all.  From block to block d grows by 20 — U' = Y + U, V' = X + V
# with 20 fresh bases each, so that either path goes on after one gap of 20 bases (-150, made good within 50 columns: no break) — and
# the band spans 2 d + ~140 diagonals: beyond the 256-diagonal window from d = 60 on, beyond the 512-diagonal one from d = 200 on.
OUTGROW_STEP = 20


def outgrow_pair(d_max, seed=7000):
    rng = np.random.default_rng(seed)
    U, V = rand_seq(rng, OUTGROW_STEP), rand_seq(rng, OUTGROW_STEP)
    a, b, d = [], [], OUTGROW_STEP
    while True:
        reps = 2 if d < 80 else 1
        a.append((U + V) * reps)
        b.append((V + U) * reps)
        if d >= d_max:
            return "".join(a), "".join(b)
        U, V, d = rand_seq(rng, OUTGROW_STEP) + U, rand_seq(rng, OUTGROW_STEP) + V, d + OUTGROW_STEP


def _outgrow_cases():
    out = []
    for d_max, holds in ((60, 512), (80, 512), (100, 512), (140, 512), (200, 0), (220, 0)):      # holds: the window that takes it (0: global memory)
        a, b = outgrow_pair(d_max, seed=7000 + d_max)
        out += _directed(f"outgrow_d{d_max}", "outgrow", a, b, what=holds)
    return out


# ---- lanes: the one-gap-per-lane kernels (FORWARD_ALIGN, both sides <= 59) and the gaps just beyond them ---------------------------
LANE_IDENTITIES = (100, 95, 85, 70, 0)


def _lanes_cases():
    out = []
    for ident in LANE_IDENTITIES:
        rng = np.random.default_rng(6800 + ident)
        a = rand_seq(rng, 140)
        b = rand_seq(rng, 140) if ident == 0 else mutate(rng, a, 10 * (100 - ident), 100 - ident)
        b = (b + rand_seq(rng, 140))[:140]
        rects = []
        for k, (n, m) in enumerate([(n, m) for n in LANE_SIDES for m in LANE_SIDES] + [(60, 10), (10, 60)]):
            o = 3 + (7 * k) % 40
            rects.append((o, o, o + n - 1, o + m - 1))
        out += _both(f"lanes_identity_{ident}", "lanes", a, b, rects, modes=(FORWARD_ALIGN,), lanes=True)
    rng = np.random.default_rng(6901)
    a = rand_seq(rng, 120)
    b = mutate(rng, a, 60, 10)
    b = (b + rand_seq(rng, 120))[:118]
    la, lb = len(a), len(b)
    an, bn = a[:20] + "N" + a[21:50] + "N" + a[51:], b[:48] + "N" + b[49:]      # rows 20 and 50, column 48
    out += _both("lanes_unclean", "lanes", an, bn, [(20, 18, 50, 40), (25, 22, 50, 47), (21, 20, 49, 48), (20, 19, 50, 48), (20, 48, 60, 70), (15, 40, 21, 48)],
                 modes=(FORWARD_ALIGN,), lanes=True)
    # the second 32-base window of a rectangle lies past the end of its stream (rows / columns / both), on the last bases
    out += _both("lanes_stream_end", "lanes", a, b, [(la - 20, lb - 50, la - 1, lb - 1), (la - 50, lb - 20, la - 1, lb - 1), (la - 20, lb - 18, la - 1, lb - 1),
                                                     (la - 33, lb - 33, la - 1, lb - 1), (la - 1, lb - 1, la - 1, lb - 1), (la - 32, lb - 40, la - 3, lb - 2)],
                 modes=(FORWARD_ALIGN,), lanes=True)
    # per size class a list of 64 k + 1 gaps, k = 0 and 2: the last wave of the class's launch has one live lane
    for cls, lo in zip(LANE_CLASSES, (1, 17, 33)):
        for k in (0, 2):
            rng = np.random.default_rng(6950 + cls + k)
            rects = []
            for t in range(64 * k + 1):
                n, m = int(rng.integers(lo, cls + 1)), int(rng.integers(1, cls + 1))
                n, m = (n, m) if t % 2 else (m, n)
                oa, ob = int(rng.integers(0, la - n + 1)), int(rng.integers(0, lb - m + 1))
                rects.append((oa, ob, oa + n - 1, ob + m - 1))
            if k == 0:
                rects = [(5, 4, 5 + cls - 1, 4 + lo - 1)]
            out.append(Case(f"lanes_list_c{cls}_k{k}", "lanes", a, b, (cls + k) % 2, rects, modes=(FORWARD_ALIGN,), lanes=True, what=cls))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = (_plain_cases() + _break_cases() + _ties_cases() + _drift_cases() + _ends_cases() + _residues_cases() + _unclean_cases() + _outgrow_cases()
           + _lanes_cases())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def lane_class(n, m):
    """The lane kernel that takes a gap of n x m bases (both boundary bases included): 16, 32, 59, or None = the wave kernel."""
    if n > PN_SMALL or m > PN_SMALL:
        return None
    return next(c for c in LANE_CLASSES if max(n, m) <= c)


# ---- the two CPU references ---------------------------------------------------------------------------------------------------------
def case_text(cs):
    """The text both host programs read."""
    text = [str(len(cs))]
    for c in cs:
        text += [f"{c.name} {c.strand} {len(c.searches)}", c.a, c.b] + [" ".join(map(str, s)) for s in c.searches]
    return "\n".join(text) + "\n"


@functools.lru_cache(maxsize=None)
def host_tool():
    """tools/anim_debug/searches, built beside its source (kept out of git) and built again only when a source is newer."""
    src = ROOT / "tools" / "anim_debug" / "searches.cpp"
    exe = src.with_suffix("")
    deps = [src, src.parent / "forced_referee.h"] + sorted((ROOT / "pyani_amd" / "csrc").glob("pg_*.h"))
    if not exe.exists() or any(d.stat().st_mtime > exe.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'pyani_amd' / 'csrc'}", f"-I{src.parent}", str(src), "-o", str(exe)], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def oracle_tool():
    sys.path.insert(0, str(ROOT))
    from oracle import oracle_build
    return oracle_build.build_nucmer_oracle()


def _emu(f):
    fit, a, b, err, score, reached, moves, down, up, wmax = (int(v) for v in f)
    return dict(fit=fit, result=(a, b, err, reached), score=score, moves=moves, down=down, up=up, wmax=wmax)


@functools.lru_cache(maxsize=None)
def expected():
    """{case name: [per search: dict(N, M, m_o, scalar=(endA, endB, errors, reached), score, wmax, e4, e8 = dict(fit, result, score,
    moves, down, up, wmax), global_errors (-1: not a lane rectangle), oracle=(endA, endB, errors, reached), ties = cells that held the
    final best score, tied_diagonals = anti-diagonals whose best score two or more cells shared)]} — one run of each host program per session."""
    cs = cases()
    text = case_text(cs)
    host = subprocess.run([str(host_tool())], input=text, capture_output=True, text=True, check=True).stdout
    orac = subprocess.run([str(oracle_tool()), "--searches"], input=text, capture_output=True, text=True, check=True).stdout
    res = {c.name: [None] * len(c.searches) for c in cs}
    by_name = {c.name: c for c in cs}
    for ln in host.splitlines():
        f = ln.split()
        name, k = f[0], int(f[1])
        assert f[2] == "scalar" and f[9] == "e4" and f[20] == "e8" and f[31] == "global" and len(f) == 33, ln
        a, b, err, score, reached, wmax = (int(v) for v in f[3:9])
        n, m = by_name[name].sides(k)
        res[name][k] = dict(N=n, M=m, m_o=by_name[name].searches[k][4], scalar=(a, b, err, reached), score=score, wmax=wmax, e4=_emu(f[10:20]), e8=_emu(f[21:31]),
                            global_errors=int(f[32]))
    for ln in orac.splitlines():
        f = ln.split()
        a, b, err, reached, ties, tied_diagonals = (int(v) for v in f[2:8])
        res[f[0]][int(f[1])].update(oracle=(a, b, err, reached), ties=ties, tied_diagonals=tied_diagonals)
    assert all(r is not None and "oracle" in r for rs in res.values() for r in rs)
    return res


def want(e, engine):
    """What pg_anim_searches returns for a search with expectation e on `engine`: (endA, endB, errors, reached, held)."""
    held = {"WALK": 1, "RUNG_GLOBAL": 1, "PREPASS": e["e4"]["fit"], "RUNG_256": e["e4"]["fit"], "RUNG_512": e["e8"]["fit"]}.get(engine)
    if engine == "LANES":      # a small gap is a lane kernel's (always answered), the others the pre-pass wave kernel's
        held = 1 if lane_class(e["N"], e["M"]) else e["e4"]["fit"]
    return e["scalar"] + (1,) if held else (0, 0, 0, 0, 0)


def list_call(strand, lanes=False, seed=91):
    """One pair of sequences holding every case of one strand back to back, and all their searches (lanes: the FORWARD_ALIGN ones) in
    shuffled order: (reference, query as stored, searches, [(case name, index, offset of the case in A, in B's strand)])."""
    cs = [c for c in cases() if c.strand == strand]
    a = "".join(c.a for c in cs)
    # strand coordinates of the concatenation: the reverse strand of b1 + b2 + ... is rc(b_k) + ... + rc(b1)
    order = cs[::-1] if strand else cs
    a_off, b_off, at = {}, {}, 0
    for c in cs:
        a_off[c.name] = at
        at += len(c.a)
    at = 0
    for c in order:
        b_off[c.name] = at
        at += len(c.b)
    b = "".join(c.b for c in cs)
    searches, who = [], []
    for c in cs:
        for k, (A0, B0, tA, tB, m_o) in enumerate(c.searches):
            if lanes and m_o != FORWARD_ALIGN:
                continue
            searches.append((A0 + a_off[c.name], B0 + b_off[c.name], tA + a_off[c.name], tB + b_off[c.name], m_o))
            who.append((c.name, k, a_off[c.name], b_off[c.name]))
    perm = np.random.default_rng(seed + strand + 2 * lanes).permutation(len(searches))
    return a, b, [searches[i] for i in perm], [who[i] for i in perm]
