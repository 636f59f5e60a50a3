"""Directed fragments for the fragment-mode (ANIb) kernels (pga_frag.inc: anib_bucket_kernel, anib_frag_kernel), with what is expected
of each: the rows of the host statement (oracle/anib_cpu.cpp, a host build of pg_anib_core.h), a CLAIM on the host statement's trace
(anib_cpu.anib_cpu_pair_trace) that says the case reaches the path it was built for, and a label that says whether the independent
blastn oracle (oracle/blastn_oracle.cpp) reports the same used rows.

A case is (name, group, query, subject, fragsize, claim); query and subject are (uint8 bases, uint64 record offsets).  Everything is
numpy with fixed seeds.  A homologous piece is an exact copy of subject bases that carries exactly the planted feature; where a flank
must not extend an alignment it is the subject's own flank with every base changed (b -> (b + 1) & 3), so that no chance match on the
alignment's diagonal moves a score.  Every group holds copies on both strands.

The numbers restated here (pg_anib_core.h): +2 a match, -3 a mismatch, a gap of k bases costs 5 + 2 k; a state more than 166 below the
best score is dead, the best score being refreshed every 4th anti-diagonal; the band holds 256 diagonals and is re-centred every 16th
anti-diagonal by an even shift of at most 8; a seed clipped to a fragment counts from 11 bases; a fragment lists at most 64 seeds, of
them at most 32 from the word tier, which leaves a strand with more than 448 word seeds alone; 8 candidates, 4 final alignments per
strand, 4 rows per fragment; an extension may use 1020 + 200 subject bases; rows pass E <= 1e-15.
"""
import collections
import functools
import math
import sys
from fractions import Fraction

import numpy as np

from tests.conftest import ROOT

for _p in (ROOT / "oracle", ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

FIELDS = ("frag", "length", "mismatch", "gaps", "nident", "qlen", "qstart", "qend", "sstart", "send", "srec", "score")
GROUPS = ("gap", "drift", "edge", "slack", "evalue", "clip", "seeds", "cands", "dirty", "ends")
Case = collections.namedtuple("Case", "name group query subject fragsize claim")
Trace = collections.namedtuple("Trace", "rows fs ext")      # rows: tuples in FIELDS order; fs / ext: anib_cpu.FS_DTYPE / EXT_DTYPE records

XDROP, BAND, MIN_CLIP, MAX_SEEDS, WORD_FIRST, WORD_MAX, MAX_CAND, MAX_FINALS, KEEP_ROWS, SLACK = 166, 256, 11, 64, 32, 448, 8, 4, 4, 200
GAP_KS = (1, 2, 8, 9, 30, 47, 48, 64, 79, 80, 81, 82, 83, 90, 120, 127, 128, 129, 200)
EVALUE_QLEN, EVALUE_DB, EVALUE_NREC, EVALUE_LS = (64, 200, 509, 1020), (3_000, 40_000, 300_000), (1, 7), tuple(range(30, 61))

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i


def bases(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)]


def changed(seq, by=1):
    """Every base changed: b -> (b + by) & 3."""
    return _ACGT[(_CODE[np.asarray(seq, dtype=np.uint8)] + by) & 3]


def revcomp(seq):
    return _ACGT[3 - _CODE[np.asarray(seq, dtype=np.uint8)]][::-1].copy()


def records(parts):
    parts = [np.ascontiguousarray(p, dtype=np.uint8) for p in parts]
    off = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), off


def substituted(seq, positions):
    out = np.array(seq, dtype=np.uint8)
    positions = np.asarray(positions, dtype=np.int64)
    out[positions] = changed(out[positions])
    return out


def rows_of(a):
    return [tuple(int(r[k]) for k in FIELDS) for r in a]


def frag_rows(t, f):
    return [r for r in t.rows if r[0] == f]


def fs_of(t, f, strand):
    return t.fs[2 * f + strand]


def exts_of(t, f, strand=None):
    return [x for x in t.ext if int(x["frag"]) == f and (strand is None or int(x["strand"]) == strand)]


@functools.lru_cache(maxsize=None)
def _subject(seed, n):
    return bases(np.random.default_rng(seed), n)


def _oriented(piece, minus):
    return revcomp(piece) if minus else piece


# ---- gap ---------------------------------------------------------------------------------------------------------------------
def _gap_locus(S, p, k, left):
    """A locus near p where a gap of k bases after `left` copied bases has one best placement: the bases next to it differ."""
    while S[p + left] == S[p + left + k] or S[p + left - 1] == S[p + left + k - 1]:
        p += 1
    return p


def _not(*avoid):
    return [b for b in _ACGT if all(b != a for a in avoid)][0]


def _gap_fragment(rng, S, p, k, kind):
    """1020 bases: an exact copy of the subject at p with ONE gap of k bases in its middle (del: k subject bases are missing from the
    query; ins: k foreign bases stand in the query).  The bases next to the gap differ, so it has one best placement."""
    if kind == "del":
        p = _gap_locus(S, p, k, 510)
        return np.concatenate([S[p:p + 510], S[p + 510 + k:p + 1020 + k]])
    left = (1020 - k) // 2
    ins = bases(rng, k)
    ins[0] = _not(S[p + left], S[p + left - 1]) if k == 1 else _not(S[p + left])
    if k > 1:
        ins[-1] = _not(S[p + left - 1])
    return np.concatenate([S[p:p + left], ins, S[p + left:p + 1020 - k]])


def _gap_claim(k, kind):
    def claim(t):
        for f in (0, 1):
            rows = frag_rows(t, f)
            if k <= 80:      # 5 + 2 k <= 165 < 166: one row bridges the gap
                assert len(rows) == 1 and rows[0][3] == k and (rows[0][6], rows[0][7]) == (1, 1020), (k, kind, f, rows)
                assert rows[0][1] == (1020 + k if kind == "del" else 1020) and rows[0][2] == 0, (k, kind, f, rows)
            elif k >= 84:    # 5 + 2 k >= 173 > 166 + 4 (a best score 4 anti-diagonals old lags by at most two matches): two rows, one per side
                # (a side may run a few chance matches into the other side's bases)
                half = 510 if kind == "del" else (1020 - k) // 2
                assert len(rows) == 2 and all(r[3] <= 3 and half - 4 <= r[4] <= half + 10 for r in rows), (k, kind, f, rows)
                assert {rows[0][6], rows[1][6]} >= {1} and {rows[0][7], rows[1][7]} >= {1020}, (k, kind, f, rows)
            else:            # 81 .. 83: next to the limit (5 + 2 k = 167 .. 171 against 166); the golden hashes pin what the statement does
                assert len(rows) in (1, 2), (k, kind, f, rows)
            pre = sum(int(fs_of(t, f, s)["rows_pre"]) for s in (0, 1))
            if 48 <= k <= 80:      # two candidates 48 or more diagonals apart grow the SAME alignment: the common-end-point rule drops one
                assert pre == 2 and len(rows) == 1, (k, kind, f, pre)
            if 8 < k <= 80:        # the best diagonal is more than one shift away: the shift is clamped (8 per re-centring)
                assert max(int(x["recentres"]) for x in exts_of(t, f)) >= (2 if k >= 30 else 1), (k, kind, f)
    return claim


def _gap_cases():
    S = _subject(101, 24_000)
    subject = records([S])
    out = []
    for kind in ("del", "ins"):
        for i, k in enumerate(GAP_KS):
            rng = np.random.default_rng([102, k, kind == "ins"])
            plus = _gap_fragment(rng, S, 1_000 + 7 * i, k, kind)
            minus = revcomp(_gap_fragment(rng, S, 12_000 + 11 * i, k, kind))
            out.append(Case(f"gap_{kind}_{k}", "gap", records([plus, minus]), subject, 1020, _gap_claim(k, kind)))
    # 81 .. 83 once more with the gap's bases a TANDEM copy of the k bases before it: the gap may open before the copy or after it, an
    # attempt at a state that lives only by what the best score has gained since its last refresh.  It is not one: a variant of the
    # statement that refreshes the best score on every anti-diagonal gives the same rows here (test_anib_frag_cases_cpu.py).  The cases
    # stay as inputs with two equal placements of a gap at the X-drop limit.
    for kind in ("del", "ins"):
        for i, k in enumerate((81, 82, 83)):
            frs, subs = [], []
            for p in (3_000 + 50 * i, 15_000 + 50 * i):
                one = S[p:p + 1020]                                                # X U Y
                two = np.concatenate([one[:510], one[510 - k:510], one[510:]])     # X U U Y
                frs.append((one if kind == "del" else two)[:1020])
                subs.append(np.concatenate([bases(np.random.default_rng([103, p]), 300), two if kind == "del" else one,
                                            bases(np.random.default_rng([104, p]), 300)]))
            out.append(Case(f"gap_{kind}_{k}_tandem", "gap", records([frs[0], revcomp(frs[1])]), records(subs), 1020, _tandem_gap_claim(k)))
    return out


def _tandem_gap_claim(k):
    def claim(t):
        for f in (0, 1):
            rows = frag_rows(t, f)
            assert len(rows) in (1, 2) and all(r[3] in (0, k) and r[2] <= 3 for r in rows) and rows[0][10] == f, (k, f, rows)
    return claim


# ---- drift -------------------------------------------------------------------------------------------------------------------
def _drift_fragment(S, p, gaps, runs, kind, every=0):
    """A 1020-base fragment over the subject from p on: an exact head (the fragment's longest exact run by far: the alignment starts
    there), then gap g of `gaps` followed by runs[i] copied bases (del: g subject bases are missing from the query; ins: g foreign
    bases stand in it).  every > 0: the copied runs carry a substitution at every `every`-th base (no exact 16-mer: no seed)."""
    pieces, s = [], p
    head = 1020 - sum(runs) - (sum(gaps) if kind == "ins" else 0)
    assert head >= 60, head
    pieces.append(S[s:s + head])
    s += head
    for g, run in zip(gaps, runs):
        if kind == "del":
            while S[s] == S[s + g] or S[s - 1] == S[s + g - 1]:      # one best placement of the gap
                pieces.append(S[s:s + 1]); s += 1; run -= 1
            s += g
        else:
            ins = changed(S[s:s + g], 2)
            ins[0] = _not(S[s])
            ins[-1] = _not(S[s - 1]) if g > 1 else _not(S[s], S[s - 1])
            pieces.append(ins)
        assert run > 0
        piece = S[s:s + run]
        last = run - 1 if s + run - p >= 1020 + (sum(gaps) if kind == "del" else -sum(gaps)) else run      # (the fragment's last base stays)
        pieces.append(substituted(piece, np.arange(every - 1, last, every)) if every else piece)
        s += run
    frag = np.concatenate(pieces)
    assert len(frag) == 1020, len(frag)
    return frag


def _drift_claim(total, far):
    def claim(t):
        for f in (0, 1):
            rows = frag_rows(t, f)
            assert rows and (rows[0][6], rows[0][7], rows[0][3]) == (1, 1020, total), (f, rows)      # the band followed the alignment to its end
            xs = [x for x in exts_of(t, f) if int(x["kind"]) >= 4]
            walked = max(xs, key=lambda x: int(x["recentres"]))
            assert int(walked["recentres"]) >= total // 8, (f, tuple(walked))                        # a shift moves at most 8 diagonals
            reach = max(abs(int(walked["lo"])), abs(int(walked["hi"])))
            assert (reach > BAND // 2) == far, (f, reach)
            assert abs(abs(int(walked["net"])) - total) <= 2, (f, tuple(walked))                     # even shifts; the last gap's 3 diagonals may be pending
    return claim


ZIGZAG_SEEDS = (879, 16240, 16870, 18905, 21199, 23795)


def _zigzag_claim(t):
    for f in range(2 * len(ZIGZAG_SEEDS)):
        assert frag_rows(t, f), f
        xs = [x for x in exts_of(t, f) if int(x["kind"]) >= 4]
        assert max(int(x["recentres"]) for x in xs) >= 8, (f, [int(x["recentres"]) for x in xs])
    both = [f for f in range(2 * len(ZIGZAG_SEEDS)) if any(int(x["lo"]) <= -8 and int(x["hi"]) >= 8 for x in exts_of(t, f))]
    assert len(both) >= 4, both      # the band went both ways within one extension


def _drift_cases():
    S = _subject(201, 30_000)
    Sr = S[::-1].copy()      # a fragment built along the reversed subject and reversed itself has its head at its END: the LEFT extension walks
    subject = records([S])
    out = []
    plans = [(45, [3] * 15, (20, 24)), (75, [3] * 25, (20, 24)), (126, [3] * 42, (20, 22)), (130, [3] * 42 + [2, 2], (20, 21)),
             (150, [3] * 50, (19, 19))]
    for total, gaps, (lo, hi) in plans:
        for kind in ("del", "ins"):
            for mirror in (False, True):
                if total in (45, 130) and mirror:
                    continue
                rng = np.random.default_rng([202, total, kind == "ins", mirror])
                frs = []
                for p in (2_000, 14_000):
                    runs = [int(r) - (3 if kind == "ins" else 0) for r in rng.integers(lo, hi + 1, size=len(gaps))]      # (ins: the same spacing in the query)
                    fr = _drift_fragment(Sr if mirror else S, p, gaps, runs, kind)
                    frs.append(fr[::-1].copy() if mirror else fr)
                name = f"drift_{kind}_{total}" + ("_left" if mirror else "")
                out.append(Case(name, "drift", records([frs[0], revcomp(frs[1])]), subject, 1020, _drift_claim(total, total > BAND // 2)))
    # Six insertions of 50 bases 54 bases apart (each earns back what it cost), then one of 80: 380 diagonals in some 1 200
    # anti-diagonals, a third of a diagonal per anti-diagonal, which a band that moved half as often would not keep up with.
    gaps, runs = [50] * 6 + [80], [54] * 6 + [150]
    frs = [_drift_fragment(S, p, gaps, runs, "ins") for p in (2_000, 9_000)]
    out.append(Case("drift_ins_380", "drift", records([frs[0], revcomp(frs[1])]), subject, 1020, _drift_claim(sum(gaps), True)))
    # Fragments that wander in both directions (zigzag_fragment; the seeds are the six of 24 000 tried whose rows a band that shifts by
    # at most 6 diagonals changes): the band is pulled back and forth and its clamped shift decides which states it still holds.
    frs = [zigzag_fragment(S, n) for n in ZIGZAG_SEEDS]
    out.append(Case("drift_zigzag", "drift", records(frs + [revcomp(f) for f in frs]), subject, 1020, _zigzag_claim))
    # a stretch that drifts faster than the band can follow (8 diagonals per 16 anti-diagonals): 6 gaps of 12 bases, 14 bases apart
    for kind in ("del", "ins"):
        gaps = [3] * 6 + [12] * 6 + [3] * 6
        runs = [22] * 6 + [14] * 5 + [60] + [22] * 6
        frs = [_drift_fragment(S, p, gaps, runs, kind) for p in (5_000, 20_000)]
        out.append(Case(f"drift_{kind}_burst", "drift", records([frs[0], revcomp(frs[1])]), subject, 1020, _drift_claim(sum(gaps), False)))
    return out


def zigzag_fragment(S, seed):
    """A fragment that wanders: exact runs of 8 .. 129 bases of the subject, between them gaps of 20 .. 85 bases in EITHER direction (a
    deletion or foreign bases), and substitutions at a rate of 0, 3 or 8 %.  The best live score changes sides with every gap."""
    rng = np.random.default_rng([205, seed])
    s, pieces, n = int(rng.integers(500, len(S) - 5_000)), [], 0
    while n < 1020:
        run = int(rng.integers(8, 130))
        pieces.append(S[s:s + run])
        s += run
        n += run
        g = int(rng.integers(20, 86))
        if int(rng.integers(0, 2)):
            s += g
        else:
            pieces.append(bases(rng, g))
            n += g
    fr = np.concatenate(pieces)[:1020]
    return substituted(fr, np.nonzero(rng.random(1020) < float(rng.choice([0, 0.03, 0.08])))[0])


# ---- edge --------------------------------------------------------------------------------------------------------------------
def _edge_claim(side, gaps):
    # Two gaps in the same direction, 60 bases apart, are both crossed (a gap of k costs 5 + 2 k, the 60 matches between them earn 120):
    # the alignment moves 120 or 140 diagonals within some 200 anti-diagonals, the band follows it by at most 8 diagonals per 16, and
    # the states left behind on the old diagonals, still live, stand on the band's first diagonal (deletions: the device keeps it in
    # lane 0) or its last (insertions: lane 63) and are shifted out there.
    def claim(t):
        for f in (0, 1):
            assert any(int(x[side]) for x in exts_of(t, f) if int(x["kind"]) >= 4), (f, [tuple(x) for x in exts_of(t, f)])
            rows = frag_rows(t, f)
            assert len(rows) == 1 and rows[0][3] == sum(gaps) and (rows[0][6], rows[0][7]) == (1, 1020), (f, rows)
    return claim


def _edge_uncrossed_claim(t):
    # Two gaps of 70 bases 40 bases apart: the 40 matches between them earn 80, less than a gap's 145, so the best cell of either side
    # lies before its first gap and the fragment has two rows without a gap.  (Whether a live state meets the band's edge here depends on the chance matches around the gaps: of eight
    # such fragments two did.  The cases above are the ones that claim it.)
    for f in (0, 1):
        rows = frag_rows(t, f)
        assert len(rows) == 2 and all(r[3] == 0 for r in rows) and {r[6] for r in rows} >= {1} and {r[7] for r in rows} >= {1020}, (f, rows)


def _edge_cases():
    S = _subject(301, 16_000)
    subject = records([S])
    out = []
    for kind, gaps, side in (("del", [60, 60], "left_low"), ("ins", [70, 70], "left_high")):
        frs = [_drift_fragment(S, p, gaps, [60, 400], kind) for p in (1_000, 9_000)]
        out.append(Case(f"edge_{kind}", "edge", records([frs[0], revcomp(frs[1])]), subject, 1020, _edge_claim(side, gaps)))
    for kind in ("del", "ins"):
        frs = [_drift_fragment(S, p, [70, 70], [40, 400], kind) for p in (3_000, 12_000)]
        out.append(Case(f"edge_{kind}_70_40", "edge", records([frs[0], revcomp(frs[1])]), subject, 1020, _edge_uncrossed_claim))
    return out


# ---- slack -------------------------------------------------------------------------------------------------------------------
def _slack_claim(total):
    def claim(t):
        for f in (0, 1):
            rows = frag_rows(t, f)
            xs = [x for x in exts_of(t, f) if int(x["kind"]) == 4]
            assert rows and len(xs) == 1 and int(fs_of(t, f, f)["cands"]) == 1, (f, rows)      # one candidate, one right extension
            used = max(int(x["dj"]) for x in xs)
            whole = len(rows) == 1 and rows[0][3] == total and (rows[0][6], rows[0][7]) == (1, 1020)
            # the start point is fragment base 1 (0-based): 1018 fragment bases lie to its right, the subject side needs `total` more
            assert whole == (1018 + total <= 1020 + SLACK), (f, total, rows)
            assert used <= 1020 + SLACK and (used == 1018 + total) == whole, (f, total, used)
    return claim


def _slack_fragment(S, p, total):
    """An exact head of 300 bases, then four deletions of about total / 4 bases (under 60 each), each followed by 180 bases that carry
    a substitution at every 12th base: the head holds the fragment's only seeds, so the one alignment grows from the head's first
    word — at subject position p = 3 mod 4 its start point is fragment base 1 — and its right extension needs 1018 + total subject
    bases."""
    assert p % 4 == 3
    cuts = [total // 4 + (1 if i < total % 4 else 0) for i in range(4)]
    assert all(c < 60 for c in cuts)
    return _drift_fragment(S, p, cuts, [180] * 4, "del", every=12)


def _short_subject_claim(n):
    def claim(t):
        for f in (0, 1):
            rows = frag_rows(t, f)
            assert len(rows) == 1 and rows[0][1] == n and {rows[0][8], rows[0][9]} == {1, n} and rows[0][2] == rows[0][3] == 0, (n, f, rows)
    return claim


def _slack_cases():
    S = _subject(401, 20_000)
    subject = records([S])
    out = []
    for total in (196, 198, 200, 202, 204):
        plus, minus = _slack_fragment(S, 2_003, total), _slack_fragment(S, 11_003, total)
        out.append(Case(f"slack_{total}", "slack", records([plus, revcomp(minus)]), subject, 1020, _slack_claim(total)))
    F = bases(np.random.default_rng(402), 1020)
    query = records([F, revcomp(F)])
    for n, lo in ((300, 360), (1019, 0), (1019, 1), (1020, 0)):
        out.append(Case(f"slack_subject_{n}_{lo}", "slack", query, records([F[lo:lo + n]]), 1020, _short_subject_claim(n)))
    return out


# ---- evalue ------------------------------------------------------------------------------------------------------------------
def length_adjustment(m, n, N):
    """BLAST_ComputeLengthAdjustment (blast_stat.c) for blastn's gapped 2 / -3 / 5 / 2 parameters, in plain floats."""
    K, logK, a_d_l, beta = 0.41, math.log(0.41), 0.8 / 0.625, -2.0
    ell_min, ell_next, converged = 0.0, 0.0, False
    a, mb, c = N, m * N + n, n * m - max(m, n) / K
    if c < 0:
        return 0
    ell_max = 2 * c / (mb + math.sqrt(mb * mb - 4 * a * c))
    ell = 0.0
    for i in range(1, 21):
        ell = ell_next
        ss = (m - ell) * (n - N * ell)
        ell_bar = a_d_l * (logK + math.log(ss)) + beta
        if ell_bar >= ell:
            ell_min = ell
            if ell_bar - ell_min <= 1.0:
                converged = True
                break
            if ell_min == ell_max:
                break
        else:
            ell_max = ell
        if ell_min <= ell_bar <= ell_max:
            ell_next = ell_bar
        else:
            ell_next = ell_max if i == 1 else (ell_min + ell_max) / 2
    adj = int(ell_min)
    if converged:
        ell = math.ceil(ell_min)
        if ell <= ell_max:
            ss = (m - ell) * (n - N * ell)
            if a_d_l * (logK + math.log(ss)) + beta >= ell:
                adj = int(ell)
    return adj


def evalue(score, m, n, N):
    adj = length_adjustment(m, n, N)
    eff_m, eff_n = max(1, m - adj), max(1, n - N * adj)
    return eff_m * eff_n * 0.41 * math.exp(-0.625 * score), eff_m, eff_n


def formula_lstar(m, n, N):
    """The smallest L in EVALUE_LS whose exact match (score 2 L) passes E <= 1e-15, by the closed formula; a value within 1e-9
    relative of the threshold is decided in exact rational arithmetic on a 60-digit exp()."""
    import decimal
    for L in EVALUE_LS:
        e, eff_m, eff_n = evalue(2 * L, m, n, N)
        if abs(e - 1e-15) <= 1e-9 * 1e-15:
            with decimal.localcontext() as ctx:
                ctx.prec = 60
                x = decimal.Decimal(eff_m * eff_n) * decimal.Decimal("0.41") * (decimal.Decimal("-0.625") * (2 * L)).exp()
            ok = Fraction(x) <= Fraction(1, 10 ** 15)
        else:
            ok = e <= 1e-15
        if ok:
            return L
    return None


def lstar_of_rows(rows):
    """(L*, monotone): fragment f of an evalue case holds the exact match of EVALUE_LS[f] bases."""
    have = sorted({r[0] for r in rows})
    if not have:
        return None, True
    return EVALUE_LS[have[0]], have == list(range(have[0], len(EVALUE_LS)))


def _evalue_subject(n, N):
    S = _subject(500 + N, 300_000)[:n]
    cut = [n * r // N for r in range(N + 1)]
    return S, records([S[cut[r]:cut[r + 1]] for r in range(N)]), cut


def _evalue_claim(m, n, N):
    def claim(t):
        lstar, monotone = lstar_of_rows(t.rows)
        assert monotone and lstar == formula_lstar(m, n, N), (m, n, N, lstar, formula_lstar(m, n, N))
        for r in t.rows:
            L = EVALUE_LS[r[0]]
            assert (r[1], r[2], r[3], r[11]) == (L, 0, 0, 2 * L), r
            assert r[10] == r[0] % N and (r[8] > r[9]) == bool(r[0] % 2), r      # the record that holds the match; odd fragments: minus strand
    return claim


def _evalue_cases():
    out = []
    for n in EVALUE_DB:
        for N in EVALUE_NREC:
            S, subject, cut = _evalue_subject(n, N)
            for m in EVALUE_QLEN:
                rng = np.random.default_rng([501, m, n, N])
                recs = []
                for i, L in enumerate(EVALUE_LS):
                    r = i % N                                          # the record that holds the exact match
                    lo, hi = cut[r], cut[r + 1]
                    a = int(rng.integers(lo, hi - L + 1))              # the match: S[a : a + L]
                    off = min(int(rng.integers(0, m - L + 1)), m - L)  # its place in the query record
                    rec = bases(rng, m)
                    s0 = a - off
                    idx = np.arange(s0, s0 + m)
                    inside = (idx >= lo) & (idx < hi)
                    rec[inside] = changed(S[idx[inside]])
                    rec[max(0, off - 12):off + L + 12] = ord("N")      # walls: no chance match next to the copy adds to its score
                    rec[off:off + L] = S[a:a + L]
                    recs.append(revcomp_dirty(rec) if i % 2 else rec)
                out.append(Case(f"evalue_q{m}_n{n}_N{N}", "evalue", records(recs), subject, m, _evalue_claim(m, n, N)))
    return out


# ---- clip --------------------------------------------------------------------------------------------------------------------
def _ninth(seq, phase=4):
    """A substitution at every 9th base: exact runs of 8, no 11-mer."""
    return substituted(seq, np.arange(phase, len(seq), 9))


def _clip_record(T, c, at_start):
    """2040 bases over the 2040-base stretch T: fragment A homologous with a substitution at every 9th base, fragment B foreign, and a
    40-base exact copy of T across their boundary with c bases in A."""
    assert len(T) == 2040
    if not at_start:      # [A | B], the exact piece ends A
        A, B = _ninth(T[:1020]), changed(T[1020:])
        rec = np.concatenate([A, B])
        rec[1020 - c:1060 - c] = T[1020 - c:1060 - c]
        rec[1020 - c - 1] = changed(T[1020 - c - 1:1020 - c])[0]
    else:                 # [B | A], the exact piece begins A
        B, A = changed(T[:1020]), _ninth(T[1020:])
        rec = np.concatenate([B, A])
        rec[980 + c:1020 + c] = T[980 + c:1020 + c]
        rec[1020 + c] = changed(T[1020 + c:1021 + c])[0]
    return rec


def _clip_claim(c, at_start):
    a = 1 if at_start else 0

    def claim(t):
        for rec in (0, 1):
            fa, fb = 2 * rec + a, 2 * rec + 1 - a
            seeds = [int(fs_of(t, fa, s)["own_seeds"]) for s in (0, 1)]
            # the clipped piece is A's only seed (clip_start_12: and one chance 16-mer far away, a lone hit that is not aligned)
            assert (seeds[rec] >= 1 and sum(seeds) <= 2 if c >= MIN_CLIP else sum(seeds) == 0) and seeds[1 - rec] == 0, (c, rec, seeds)
            rows = frag_rows(t, fa)
            assert (len(rows) == 1) == (c >= MIN_CLIP) and len(rows) <= 1, (c, rec, rows)
            if rows:
                assert rows[0][1] > 900 and (rows[0][8] > rows[0][9]) == bool(rec), rows
            assert int(fs_of(t, fb, rec)["own_seeds"]) == 1 and not frag_rows(t, fb), (c, rec)      # 40 - c bases: below the e-value cut
    return claim


LAST_FRAGMENTS = (1, 10, 11, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def _last_claim(minus):
    def claim(t):
        for i, r in enumerate(LAST_FRAGMENTS):
            f = 2 * i + 1
            rows = frag_rows(t, f)
            fs = fs_of(t, f, int(minus))
            assert int(fs["own_seeds"]) == (1 if r >= MIN_CLIP else 0), (r, tuple(fs))
            if r >= 63:
                assert len(rows) == 1 and rows[0][1] == r == rows[0][5] and (rows[0][6], rows[0][7]) == (1, r), (r, rows)
            if r <= 17:
                assert not rows, (r, rows)
            assert len(frag_rows(t, f - 1)) == 1
    return claim


def _clip_cases():
    S = _subject(601, 60_000)
    subject = records([S])
    out = []
    for at_start in (False, True):
        for c in (10, 11, 12):
            p = 1_000 + 4_500 * (c - 10) + 15_000 * at_start
            plus = _clip_record(S[p:p + 2040], c, at_start)
            minus = _clip_record(revcomp(S[p + 2_100:p + 4_140]), c, at_start)
            out.append(Case(f"clip_{'start' if at_start else 'end'}_{c}", "clip", records([plus, minus]), subject, 1020, _clip_claim(c, at_start)))
    for minus in (False, True):
        recs = []
        for i, r in enumerate(LAST_FRAGMENTS):
            p = 32_000 + 1_100 * i + 14_000 * minus
            piece = S[p:p + 1020 + r]
            recs.append(revcomp(piece) if minus else piece)
        out.append(Case(f"clip_last_{'minus' if minus else 'plus'}", "clip", records(recs), subject, 1020, _last_claim(minus)))
    return out


# ---- seeds -------------------------------------------------------------------------------------------------------------------
def _seeds_repeat_case(name, elen, seed):
    """A fragment whose own seeds outnumber the list: an element of `elen` bases stands at 40 subject loci and 3 times in the fragment
    (120 seeds of equal length: the cut falls inside the ties); the fragment's true locus is diverged about 15 %, its seeds are
    shorter than the element's and rank below the cut."""
    rng = np.random.default_rng(seed)
    E = bases(rng, elen)
    F = bases(rng, 1020)
    places = (100, 480, 860)
    for q in places:
        F[q:q + elen] = E
        F[q - 1], F[q + elen] = changed(E[:1], 1)[0], changed(E[-1:], 1)[0]
    parts = []
    for i in range(40):
        spacer = bases(rng, 700)
        spacer[-1] = changed(E[:1], 2)[0]      # the subject's flanks differ from the fragment's: the match is elen bases exactly
        parts += [spacer, E, changed(E[-1:], 2)]
    true = _runs(F, [20, 4, 4, 4, 4, 4])      # 13 %: 22 seeds of 20 bases, equal among themselves and shorter than the element's
    for q in places:
        true[q:q + elen] = changed(E, 3)      # the true locus holds no copy of the element
    parts += [bases(rng, 500), true, bases(rng, 500)]
    subject = records([np.concatenate(parts)])
    cands = 2 if 2 * elen < 128 else MAX_CAND      # candidates beyond the second need an initial HSP of 128

    def claim(t):
        for f in (0, 1):
            fs = fs_of(t, f, f)
            assert int(fs["own_seeds"]) >= 120 > MAX_SEEDS == int(fs["listed"]), tuple(fs)
            assert int(fs["cands"]) == cands and int(fs["finals"]) == min(cands, MAX_FINALS), tuple(fs)
            assert len(frag_rows(t, f)) == (min(cands, KEEP_ROWS) if 2 * elen >= 90 else 0), frag_rows(t, f)
    return Case(name, "seeds", records([F, revcomp(F)]), subject, 1020, claim)


def _runs(seq, lengths):
    """Substitutions that leave exact runs of the given lengths (cycled), one substituted base between two runs."""
    pos, at, i = [], 0, 0
    while True:
        at += lengths[i % len(lengths)]
        if at >= len(seq):
            break
        pos.append(at)
        at += 1
        i += 1
    return substituted(seq, pos)


def _seeds_word_case():
    """The word tier (it runs when some but not all fragments of the pair report).  Fragment 0 reports; 1 fails with 1 .. 31 word
    seeds; 2 with 33 .. 448; 3 with more than 448 (a low-complexity stretch against many such loci); 4 has one word, a piece of its own
    seed; 5 has a true locus in runs of 11 whose words rank below the 23 longer words (runs of 13) of a 330-base decoy."""
    rng = np.random.default_rng(702)
    S = bases(rng, 30_000)
    lowc = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 40)
    for i in range(24):
        S[20_000 + 300 * i:20_000 + 300 * i + 80] = lowc
    f5 = S[10_000:11_020].copy()
    S[10_000:11_020] = _runs(f5, [11])
    S[12_000:12_330] = _runs(f5[300:630], [13])
    f0 = S[1_000:2_020].copy()
    f1 = _runs(S[3_000:4_020], [8, 8, 8, 8, 12, 8, 8, 8, 8, 13, 8, 8, 8, 8, 14, 8, 8, 8, 8, 15])      # 20 runs of 12 .. 15 among runs of 8
    f2 = _runs(S[5_000:6_020], [12])                                                                    # 78 runs of 12
    f3 = bases(rng, 1020)
    f3[400:460] = lowc[:60]
    f4 = np.concatenate([S[8_000:8_500], changed(S[8_500:9_020])])
    frs = [f0, f1, f2, f3, f4, f5]
    query = records(frs + [revcomp(f) for f in frs])
    subject = records([S])

    def claim(t):
        for base, strand in ((0, 0), (6, 1)):
            g = lambda f: fs_of(t, base + f, strand)      # noqa: E731
            assert int(g(0)["word_found"]) == 0 and len(frag_rows(t, base)) >= 1
            assert 1 <= int(g(1)["word_found"]) <= 31 and int(g(1)["word_taken"]) == int(g(1)["word_found"]) and int(g(1)["own_seeds"]) == 0, tuple(g(1))
            assert WORD_FIRST < int(g(2)["word_found"]) <= WORD_MAX and int(g(2)["word_taken"]) == WORD_FIRST, tuple(g(2))
            assert int(g(3)["word_found"]) > WORD_MAX and int(g(3)["word_taken"]) == 0 and int(g(3)["own_seeds"]) > MAX_SEEDS, tuple(g(3))
            assert int(g(4)["word_found"]) >= 1 and int(g(4)["word_taken"]) == 0 and int(g(4)["own_seeds"]) == 1, tuple(g(4))
            assert int(g(5)["word_found"]) > WORD_FIRST + 23 and int(g(5)["word_taken"]) == WORD_FIRST, tuple(g(5))
            for f in (1, 2, 5):
                rows = frag_rows(t, base + f)
                assert rows and rows[0][1] > 900, (f, rows)      # found by the word tier
    return Case("seeds_word_tier", "seeds", query, subject, 1020, claim)


def _seeds_cases():
    return [_seeds_repeat_case("seeds_repeat_30", 30, 701), _seeds_repeat_case("seeds_repeat_48", 48, 703),
            _seeds_repeat_case("seeds_repeat_70", 70, 704), _seeds_word_case()]


# ---- cands -------------------------------------------------------------------------------------------------------------------
def _cands_case():
    """One fragment with 10 loci on the plus and 3 on the minus strand, 2 % .. 20 % diverged: more than 8 candidates, 4 final alignments
    per strand and 4 rows.  A locus is the fragment with a substitution at every e-th base (e = 5 .. 16: no exact 16-mer) and three
    exact stretches of 50 bases, which are its seeds; the closest locus (e = 50) is seeded by its runs of 49.  57 seeds in all: every
    locus is in the list."""
    rng = np.random.default_rng(801)
    F = bases(rng, 1020)
    order = [(e, False) for e in (50, 13, 12, 11, 10, 9, 8, 7, 6, 5)] + [(e, True) for e in (16, 15, 14)]
    parts = [bases(rng, 900)]
    for n, j in enumerate(rng.permutation(len(order))):
        e, minus = order[int(j)]
        pos = np.arange(e - 1, 1020, e)
        if e != 50:
            keep = np.ones(1020, dtype=bool)
            for q in (40 + 17 * n, 380 + 17 * n, 720 + 17 * n):      # the exact stretches, walled by a substitution on either side
                keep[q:q + 50] = False
                pos = np.concatenate([pos, [q - 1, q + 50]])
            pos = np.unique(pos[keep[pos]])
        copy = substituted(F, pos)
        parts += [revcomp(copy) if minus else copy, bases(rng, 900)]
    subject = records([np.concatenate(parts)])

    def claim(t):
        for f, own in ((0, 0), (1, 1)):
            a, b = fs_of(t, f, own), fs_of(t, f, 1 - own)      # the strand with 10 loci, the one with 3
            assert int(a["own_seeds"]) + int(b["own_seeds"]) == 57 and int(a["listed"]) == 48, (tuple(a), tuple(b))
            assert int(a["cands"]) == MAX_CAND and int(a["prelims"]) >= MAX_CAND and int(a["finals"]) == MAX_FINALS, tuple(a)
            assert int(b["cands"]) == 3 == int(b["finals"]), tuple(b)
            assert int(a["rows_pre"]) + int(b["rows_pre"]) == 7 and len(frag_rows(t, f)) == KEEP_ROWS, (tuple(a), tuple(b))
            scores = [r[11] for r in frag_rows(t, f)]
            assert scores == sorted(scores, reverse=True) and len(set(scores)) == 4 and len({r[8] > r[9] for r in frag_rows(t, f)}) == 2, frag_rows(t, f)
    return Case("cands_13_loci", "cands", records([F, revcomp(F)]), subject, 1020, claim)


def _regular_locus(F, e, n):
    """F with a substitution at every e-th base and three exact stretches of 50 bases (its seeds), walled by a substitution."""
    pos = np.arange(e - 1, 1020, e)
    keep = np.ones(1020, dtype=bool)
    for q in (40 + 17 * n, 380 + 17 * n, 720 + 17 * n):
        keep[q:q + 50] = False
        pos = np.concatenate([pos, [q - 1, q + 50]])
    return substituted(F, np.unique(pos[keep[pos]]))


def _shared_end_case():
    """Two loci that share ONE end point.  The fragment ends in two copies of a 60-base unit (A U U) and the subject holds three
    (A U U U): beside the main row on diagonal 0 the fragment's two units match the subject's last two, 120 exact bases 60 diagonals
    away, a candidate of their own whose left extension crosses a 60-base gap into the main alignment and runs with it to the main
    row's first base - the same start point, another end and a lower score.  The common-end-point rule drops that row.  Three further
    loci (a substitution at every 12th, 9th, 7th base, the last on the other strand) make five rows before the cuts: the four best are
    kept first, then the rule takes its one, and three remain.  Fragment 0 / 1: plus / minus strand.  Fragments 2 / 3 are the mirror
    image (U U A against U U U A): the second candidate crosses on its RIGHT and shares the main row's END point only."""
    rng = np.random.default_rng(802)
    frs, recs = [], []
    for i in range(4):
        A, U = bases(rng, 900), bases(rng, 60)
        U[0], U[-1] = _not(A[-1], U[-1]), _not(A[0], U[0], U[-1])      # the units are walled: no match runs from A into a unit's copy
        F = np.concatenate([A, U, U] if i < 2 else [U, U, A])
        main = np.concatenate([A, U, U, U] if i < 2 else [U, U, U, A])
        parts = [bases(rng, 700), main]
        for n, e in enumerate((12, 9, 7)):      # the third one on the other strand: a strand makes at most 4 final alignments
            parts += [bases(rng, 700), revcomp(_regular_locus(F, e, n)) if e == 7 else _regular_locus(F, e, n)]
        parts.append(bases(rng, 700))
        frs.append(revcomp(F) if i % 2 else F)
        recs.append(np.concatenate(parts))

    def claim(t):
        for f in range(4):
            rows = frag_rows(t, f)
            pre = sum(int(fs_of(t, f, s)["rows_pre"]) for s in (0, 1))
            assert pre >= 5 and int(fs_of(t, f, f % 2)["finals"]) == MAX_FINALS == int(fs_of(t, f, f % 2)["rows_pre"]), (f, pre, rows)
            assert (rows[0][1], rows[0][2], rows[0][3], rows[0][10]) == (1020, 0, 0, f) and all(r[3] == 0 and r[10] == f for r in rows), (f, rows)
            # the dropped row, read from the trace: an extension that crossed the 60-base gap and reached the main row's first (left
            # extension, kind 5) or last base (right extension, kind 4), and was not cut back by the second look
            crossed = [int(x["kind"]) for x in exts_of(t, f) if abs(int(x["di"]) - int(x["dj"])) == 60 and int(x["di"]) >= 890 and int(x["score"]) > 1500]
            assert crossed and set(crossed) <= ({5, 6} if f < 2 else {4, 7}), (f, crossed)
            assert len(rows) == 3 < KEEP_ROWS and {r[8] > r[9] for r in rows} == {bool(f % 2)}, (f, rows)      # the other strand's rows fell to the 4-row cap, before the rule
    return Case("cands_shared_end", "cands", records(frs), records(recs), 1020, claim)


# ---- dirty -------------------------------------------------------------------------------------------------------------------
def _dirty_case(minus):
    """N runs of 1, 5 and 40 bases and lowercase bases in query and subject; the runs start at positions = 0, 15, 16, 31 mod 32, next to
    a fragment's only seed, and at a fragment's first and last base."""
    rng = np.random.default_rng([901, minus])
    S = bases(rng, 12_000)
    src = revcomp(S) if minus else S                 # query coordinates run along src
    f0 = src[1_024:2_044].copy()                     # exact, with N runs in the query
    runs0 = [(0, 1), (15, 5), (32 * 3 + 16, 40), (32 * 6 + 31, 1), (32 * 9, 5), (32 * 12 + 15, 40), (32 * 16 + 16, 1), (32 * 20 + 31, 5), (1019, 1)]
    for q, n in runs0:
        f0[q:q + n] = ord("N")
    f1 = _ninth(src[3_072:4_092])                    # one seed of 20 bases, an N on either side of it
    f1[500:520] = src[3_572:3_592]
    f1[520] = ord("N")
    f1[499] = ord("N")
    f2 = src[5_120:6_140].copy()                     # exact, lowercase in places; the N runs are in the subject
    low = rng.random(1020) < 0.4
    f2[low] += 32
    f3 = _ninth(src[7_168:8_188])                    # one seed of 20 bases, the SUBJECT has an N right behind it
    f3[300:320] = src[7_468:7_488]
    f3[299], f3[320] = changed(src[7_467:7_468])[0], changed(src[7_488:7_489])[0]
    Sd = src.copy()
    for q, n in ((5_120 + 32 * 2, 1), (5_120 + 32 * 5 + 15, 40), (5_120 + 32 * 9 + 16, 5), (5_120 + 32 * 14 + 31, 40), (5_120 + 32 * 20, 5),
                 (5_120 + 32 * 25 + 15, 1), (7_488, 1), (7_467, 1)):
        Sd[q:q + n] = ord("N")
    lows = rng.random(len(Sd)) < 0.3
    Sd[lows & (Sd != ord("N"))] += 32
    subject = records([revcomp_dirty(Sd) if minus else Sd])
    strand = int(minus)

    def claim(t):
        r0, r1, r2, r3 = (frag_rows(t, f) for f in range(4))
        assert r0 and (r0[0][6], r0[0][7]) == (2, 1019) and r0[0][2] == sum(n for _, n in runs0) - 2 and r0[0][3] == 0, r0
        assert int(fs_of(t, 1, strand)["own_seeds"]) == 1 and r1 and r1[0][2] >= 100 and r1[0][1] > 900, (tuple(fs_of(t, 1, strand)), r1)
        assert r2 and (r2[0][6], r2[0][7]) == (1, 1020) and r2[0][2] == 1 + 40 + 5 + 40 + 5 + 1 and r2[0][3] == 0, r2
        assert int(fs_of(t, 3, strand)["own_seeds"]) == 1 and r3 and r3[0][1] > 900, (tuple(fs_of(t, 3, strand)), r3)
        assert all((r[8] > r[9]) == bool(minus) for r in t.rows), t.rows
    return Case(f"dirty_{'minus' if minus else 'plus'}", "dirty", records([f0, f1, f2, f3]), subject, 1020, claim)


def revcomp_dirty(seq):
    """Reverse complement that keeps N and letter case."""
    seq = np.asarray(seq, dtype=np.uint8)
    out = seq[::-1].copy()
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    return comp[out]


# ---- ends --------------------------------------------------------------------------------------------------------------------
def _ends_cases():
    from tests import anib_search_cases as sc
    out = []
    q, s = sc.ends_case()

    def ends_claim(t):
        starts = {(r[10], min(r[8], r[9])) for r in t.rows}
        ends = {(r[10], max(r[8], r[9])) for r in t.rows}
        assert ((0, 1) in starts or (1, 1) in starts) and ((0, 20_000) in ends or (1, 20_000) in ends) and {r[10] for r in t.rows} == {0, 1}
    out.append(Case("ends_diverged", "ends", q, s, 1020, ends_claim))
    q, s = sc.tandem_case()

    def tandem_claim(t):
        frags = [r[0] for r in t.rows]
        assert max(frags.count(f) for f in set(frags)) >= 2
    out.append(Case("ends_tandem", "ends", q, s, 1020, tandem_claim))
    seq = _subject(1001, 40_000)
    subject = (seq, np.array([0, 20_000, 40_000], dtype=np.uint64))
    junction = seq[19_280:21_320]      # fragment 0: 720 bases of record 0 and 300 of record 1, contiguous in the file; fragment 1: record 1
    first, last = seq[:1020], seq[38_980:]
    for minus in (False, True):
        recs = [_oriented(x, minus) for x in (junction, first, last)]

        def claim(t, minus=minus):
            fj = 1 if minus else 0                                   # the fragment that straddles the junction
            rows = frag_rows(t, fj)
            # the alignment stops at the record's last base; the 300 bases in the next record are another subject sequence, and only
            # the best one's is reported (-max_target_seqs 1)
            assert len(rows) == 1 and rows[0][10] == 0 and rows[0][1] == 720 and max(rows[0][8], rows[0][9]) == 20_000, rows
            other = frag_rows(t, 1 - fj)
            assert len(other) == 1 and other[0][10] == 1 and other[0][1] == 1020, other
            r_first, r_last = frag_rows(t, 2), frag_rows(t, 3)
            assert len(r_first) == 1 and r_first[0][10] == 0 and min(r_first[0][8], r_first[0][9]) == 1 and r_first[0][1] == 1020, r_first
            assert len(r_last) == 1 and r_last[0][10] == 1 and max(r_last[0][8], r_last[0][9]) == 20_000 and r_last[0][1] == 1020, r_last
        out.append(Case(f"ends_junction_{'minus' if minus else 'plus'}", "ends", records(recs), subject, 1020, claim))
    # the other side of the junction: 300 bases of record 0, then 720 of record 1 - the row starts at record 1's first base
    for minus in (False, True):
        def claim(t):
            rows = frag_rows(t, 0)
            assert len(rows) == 1 and rows[0][10] == 1 and rows[0][1] == 720 and min(rows[0][8], rows[0][9]) == 1, rows
        out.append(Case(f"ends_junction_record1_{'minus' if minus else 'plus'}", "ends", records([_oriented(seq[19_700:20_720], minus)]),
                        subject, 1020, claim))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    out = (_gap_cases() + _drift_cases() + _edge_cases() + _slack_cases() + _evalue_cases() + _clip_cases() + _seeds_cases()
           + [_cands_case(), _shared_end_case()] + [_dirty_case(False), _dirty_case(True)] + _ends_cases())
    assert len({c.name for c in out}) == len(out) and {c.group for c in out} == set(GROUPS)
    return tuple(out)


def by_group(group):
    return [c for c in all_cases() if c.group == group]


# ---- the independent oracle --------------------------------------------------------------------------------------------------
# Whether the rows parse_blast_tab uses (coverage > 70 %) are those of oracle/blastn_oracle.cpp; set after running both, and asserted
# either way (tests/test_anib_frag_cases_cpu.py), so a label cannot go stale.  Every case not named here is "equal".
_XDROP_PATH = ("differs: one strand's row has the oracle's extent and gap but fewer mismatches and a higher score - the statement walks "
               "anti-diagonals and compares with a best score refreshed every 4th, blastn walks rows and compares with the row's own best, "
               "so next to the X-drop limit (a gap of 81 or 82 bases costs 167 or 169 against 166) they keep different paths alive")
ORACLE = {
    "gap_del_81": _XDROP_PATH, "gap_del_82": _XDROP_PATH, "gap_ins_82": _XDROP_PATH, "gap_del_82_tandem": _XDROP_PATH,
    "gap_ins_82_tandem": _XDROP_PATH,
    "drift_zigzag": "differs: the wandering fragments align in several pieces of under 70 % each; the statement reports 2 used rows, blastn 4",
    "edge_ins": "differs: one strand's row differs in the mismatches around the two 70-base insertions (the same limit, two gaps deep)",
    "slack_204": "differs: the statement's extension may use 1020 + 200 subject bases and stops 2 bases short; blastn has no such cap",
    "seeds_repeat_30": "differs: the 64-seed list holds only the element's 120 seeds, the true locus (seeds of 20) is cut; blastn finds it",
    "seeds_repeat_48": "differs: the 64-seed list holds only the element's 120 seeds, the true locus (seeds of 20) is cut; blastn finds it",
    "seeds_repeat_70": "differs: the 64-seed list holds only the element's 120 seeds, the true locus (seeds of 20) is cut; blastn finds it",
}


def oracle_label(case):
    return ORACLE.get(case.name, "equal")


# ---- the golden hashes -------------------------------------------------------------------------------------------------------
GOLDEN = ROOT / "tests" / "golden" / "anib_frag_cases_sha1.txt"


def rows_sha1(rows):
    import hashlib
    return hashlib.sha1("\n".join(" ".join(str(v) for v in r) for r in rows).encode()).hexdigest()


def golden_text():
    """One line per case: name, number of rows, sha1 of the host statement's rows (12 fields a row, in order)."""
    return "".join(f"{c.name} {len(host_trace(c).rows)} {rows_sha1(host_trace(c).rows)}\n" for c in all_cases())


# ---- references --------------------------------------------------------------------------------------------------------------
_trace, _oracle = {}, {}


def host_trace(case):
    """Trace(rows, fs, ext) of the host statement in the default search, once per process; callers do not modify it."""
    if case.name not in _trace:
        import anib_cpu
        rows, fs, ext = anib_cpu.anib_cpu_pair_trace(case.query, case.subject, case.fragsize)
        _trace[case.name] = Trace(rows_of(rows), fs, ext)
    return _trace[case.name]


def host_pair(monkeypatch, case, mode="seeds", defines=None):
    """The host statement's rows (tuples) of one case in `mode`, or of the variant built with `defines`.  This function owns the
    variable that switches the statement's search (tests/anib_search_cases.py): it is gone again when the call returns."""
    import os
    import anib_cpu
    from tests import anib_search_cases as sc
    assert mode in sc.MODES
    if mode == "all_diagonals":
        monkeypatch.setenv(sc.ENV, "1")
    else:
        monkeypatch.delenv(sc.ENV, raising=False)
    try:
        return rows_of(anib_cpu.anib_cpu_pair(case.query, case.subject, case.fragsize, defines=defines))
    finally:
        monkeypatch.delenv(sc.ENV, raising=False)
        assert sc.ENV not in os.environ


def oracle_rows(case):
    """Every row of the independent blastn oracle's table (numpy records), once per process."""
    if case.name not in _oracle:
        import blastn_oracle
        _oracle[case.name] = blastn_oracle.blastn_pair(case.query, case.subject, case.fragsize)
    return _oracle[case.name]


def used_equal(rows, case):
    """Whether the rows parse_blast_tab uses of `rows` (numpy records or tuples in FIELDS order) are the oracle's used rows."""
    import blastn_oracle_agreement as agreement
    from anib_product_vs_oracle import side_by_side, tuples
    if len(rows) and not hasattr(rows[0], "dtype"):
        rows = [dict(zip(FIELDS, r)) for r in rows]
    up, uo = agreement.used_rows(tuples(rows)), agreement.used_rows(tuples(oracle_rows(case)))
    rep = side_by_side(up, uo)
    return rep["identical"] == rep["used_rows_other"] == rep["used_rows_product"], rep


if __name__ == "__main__":      # python -m tests.anib_frag_cases --write-golden: after a deliberate change of the host statement
    if "--write-golden" in sys.argv:
        GOLDEN.write_text(golden_text())
        print(f"wrote {GOLDEN}")
