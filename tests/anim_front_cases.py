"""Directed cases for the ANIm front end: seeding (pga_seed.inc) and the cluster stage (pga_cluster.inc: MUM filter, mgaps
clustering, chain extraction) at their own thresholds — a match of exactly 20 bases, a query gap of exactly 90, a diagonal
difference of exactly max(5, int(0.12 * sep)), a cluster of exactly 65 matched bases — which generator genomes meet only by
chance.  tests/test_anim_front_cpu.py holds every case against the nucmer oracle and the host statement, tests/test_anim_front_gpu.py
holds the device code against the oracle.

A case is a pair of small genomes (A, B) built from seeded random filler with exact matches planted in it, and per mode (--mum,
--maxmatch) and direction (A as reference, B as reference) a CLAIM: the planted clusters that must come out as alignment
records — one record per cluster, no other record; an empty list claims "no record at all".

The builder forces a mismatch (or meets a sequence end / an ambiguity symbol) on both flanks of every planted match and between
the runs of a core, and then VERIFIES on the finished sequences that every planted match is maximal exactly as planted, in
reference-stream and query-STRAND-stream coordinates (records joined by one separator; position p of the reverse strand is the
complement of base len - 1 - p: the coordinates the seeding kernels sample in).  A random filler base that continued a planted
match would move a threshold (gap 91 becomes 90) — here that is an AssertionError while the cases are built."""
import functools
import random
import subprocess
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

MIN_MATCH, MIN_CLUSTER, MAX_GAP, DIAG_DIFF, DIAG_FACTOR = 20, 65, 90, 5, 0.12      # nucmer -l -c -g -D -d as pyani runs it
SEED_STEP, MASK_WORD = 5, 32      # the query strand is sampled at every 5th position; clean-mask words hold 32 reference positions
SLACK = 40                        # an alignment may run on past a forced mismatch where the filler happens to agree for a few bases
_COMP = str.maketrans("ACGTN", "TGCAN")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def joins(sep, dd):
    """mgaps' join rule for two matches: query gap sep, diagonal difference dd."""
    return sep <= MAX_GAP and dd <= max(DIAG_DIFF, int(DIAG_FACTOR * sep))


# (sep, dd, joined) as the oracle resolves them
JOIN_TABLE = [(90, 0, 1), (91, 0, 0), (30, 5, 1), (30, 6, 0), (41, 5, 1), (49, 6, 0), (50, 6, 1), (75, 9, 1), (75, 10, 0),
              (84, 10, 1), (84, 11, 0), (90, 10, 1), (90, 11, 0)]
assert all(joins(s, d) == bool(j) for s, d, j in JOIN_TABLE)
# (match lengths, record?) with query gap 30, diagonal difference 0
MIN_CLUSTER_TABLE = [((32, 32), 0), ((32, 33), 1), ((20, 44), 0), ((20, 45), 1), ((64,), 0), ((65,), 1), ((21, 21, 22), 0), ((21, 22, 22), 1)]
MANY_FORMS = [(90, 0), (91, 0), (75, 9), (75, 10)]      # the forms the clusters of family 6 cycle through
MANY_CLUSTERS = 300
FAMILIES = {1: "seed phases", 2: "position edges", 3: "join thresholds", 4: "minimum cluster", 5: "MUM uniqueness", 6: "many clusters in one unit"}


@dataclass
class Planted:      # one planted maximal match, verified on the finished sequences
    r: int          # reference stream position
    q: int          # query STRAND stream position
    len: int
    strand: int
    rrec: int
    rpos: int       # position in the reference record
    qrec: int
    qpos: int       # FORWARD position in the query record


@dataclass
class Case:
    name: str
    family: int
    ref: list                                   # [(record id, sequence)] of genome A
    qry: list                                   # of genome B
    expect: dict = field(default_factory=dict)  # (maxmatch, swapped) -> [cluster]: (a_rec, a_lo, a_hi, b_rec, b_lo, b_hi, strand), forward, half-open
    planted: list = field(default_factory=list)


class _Pair:
    """Two genomes of random filler; plant() writes a match and locks what it wrote and the flanks it forced."""

    def __init__(self, seed, ref_lens, qry_lens):
        self.rng = random.Random(seed)
        self.seq = [[[self.rng.choice("ACGT") for _ in range(n)] for n in lens] for lens in (ref_lens, qry_lens)]
        self.lock = [[set() for _ in lens] for lens in (ref_lens, qry_lens)]
        self.runs = []      # (rrec, rpos, qrec, strand position in the record, length, strand)

    def _put(self, side, rec, pos, text):
        s, lk = self.seq[side][rec], self.lock[side][rec]
        assert 0 <= pos and pos + len(text) <= len(s), ("planted text leaves its record", side, rec, pos, len(text), len(s))
        for i, c in enumerate(text):
            assert pos + i not in lk or s[pos + i] == c, ("two plants disagree on a base", side, rec, pos + i)
            s[pos + i] = c
            lk.add(pos + i)

    def put_strand(self, rec, spos, text, strand):
        """Write text into query record rec as it reads on the strand, from strand position spos."""
        n = len(self.seq[1][rec])
        self._put(1, rec, spos if strand == 0 else n - spos - len(text), text if strand == 0 else revcomp(text))

    def put_ref(self, rec, pos, text):
        self._put(0, rec, pos, text)

    def _force_mismatch(self, rrec, rp, qrec, sp, strand):
        """Reference position rp meets query strand position sp on a flank of a match: make them differ, unless one of them is absent."""
        R, Q = self.seq[0][rrec], self.seq[1][qrec]
        if not (0 <= rp < len(R) and 0 <= sp < len(Q)):
            return
        f = sp if strand == 0 else len(Q) - 1 - sp
        qb = Q[f] if strand == 0 else Q[f].translate(_COMP)
        if R[rp] == qb and qb != "N":
            if f not in self.lock[1][qrec]:
                b = self.rng.choice([c for c in "ACGT" if c != R[rp]])
                Q[f] = b if strand == 0 else b.translate(_COMP)
            else:
                assert rp not in self.lock[0][rrec], ("both flank bases are taken and agree", rrec, rp, qrec, sp)
                R[rp] = self.rng.choice([c for c in "ACGT" if c != qb])
        self.lock[0][rrec].add(rp)
        self.lock[1][qrec].add(f)

    def plant(self, rrec, rpos, qrec, spos, rtext, qtext=None, strand=0):
        """rtext at reference position rpos, qtext (default: the same) at query strand position spos; both in reference orientation.
        Where the two texts differ the match is cut: every stretch on which they agree becomes one planted match."""
        qtext = rtext if qtext is None else qtext
        T = len(rtext)
        assert len(qtext) == T
        self.put_ref(rrec, rpos, rtext)
        self.put_strand(qrec, spos, qtext, strand)
        self._force_mismatch(rrec, rpos - 1, qrec, spos - 1, strand)
        self._force_mismatch(rrec, rpos + T, qrec, spos + T, strand)
        o = 0
        while o < T:
            e = o
            while e < T and rtext[e] == qtext[e]:
                e += 1
            if e > o:
                self.runs.append((rrec, rpos + o, qrec, spos + o, e - o, strand))
            o = max(e, o + 1)

    def finish(self):
        """([(id, sequence)] of A, of B, [Planted]) — after checking every planted match on the finished sequences."""
        ref = ["".join(s) for s in self.seq[0]]
        qry = ["".join(s) for s in self.seq[1]]
        R = "#".join(ref)
        S = ["#".join(qry), "#".join(revcomp(s) for s in reversed(qry))]
        rstart = [sum(len(s) + 1 for s in ref[:k]) for k in range(len(ref))]
        qstart = [[sum(len(s) + 1 for s in qry[:k]) for k in range(len(qry))],
                  [sum(len(s) + 1 for s in qry[k + 1:]) for k in range(len(qry))]]
        out = []
        for rrec, rpos, qrec, spos, n, strand in self.runs:
            r, q, Q = rstart[rrec] + rpos, qstart[strand][qrec] + spos, S[strand]
            assert R[r:r + n] == Q[q:q + n] and len(R[r:r + n]) == n and set(R[r:r + n]) <= set("ACGT"), ("planted match is not exact", rrec, rpos, n)

            def open_end(i, j):      # may the match run on over reference position i / strand position j?
                return 0 <= i < len(R) and 0 <= j < len(Q) and R[i] == Q[j] and R[i] in "ACGT"
            assert not open_end(r - 1, q - 1), ("planted match is not left-maximal", rrec, rpos, qrec, spos, strand)
            assert not open_end(r + n, q + n), ("planted match is not right-maximal", rrec, rpos, qrec, spos, strand)
            out.append(Planted(r, q, n, strand, rrec, rpos, qrec, spos if strand == 0 else len(qry[qrec]) - spos - n))
        return [(f"a{k}", s) for k, s in enumerate(ref)], [(f"b{k}", s) for k, s in enumerate(qry)], out


def _cluster(ms):
    """The planted matches ms as one expected record."""
    assert len({(m.rrec, m.qrec, m.strand) for m in ms}) == 1
    return (ms[0].rrec, min(m.rpos for m in ms), max(m.rpos + m.len for m in ms),
            ms[0].qrec, min(m.qpos for m in ms), max(m.qpos + m.len for m in ms), ms[0].strand)


def _core(rng, run_len, n_runs=4):
    """n_runs exact runs with single forced mismatches between them: (reference text, query text)."""
    rt, qt = [], []
    for k in range(n_runs):
        run = "".join(rng.choice("ACGT") for _ in range(run_len))
        rt.append(run)
        qt.append(run)
        if k + 1 < n_runs:
            x = rng.choice("ACGT")
            rt.append(x)
            qt.append(rng.choice([c for c in "ACGT" if c != x]))
    return "".join(rt), "".join(qt)


def _same_everywhere(clusters):
    return {(mm, sw): list(clusters) for mm in (False, True) for sw in (False, True)}


# ---- family 1: seed phases ------------------------------------------------------------------------------------------
def _sheet(name, seed, strand, run_lens, rstep, qstep, qtail, record):
    """One core per entry of run_lens (four runs of that length): core i at reference position r0 + i * rstep and query strand
    position q0 + i * qstep.  rstep = 1 mod 32 and qstep = 1 mod 5, so 160 cores meet every (reference start mod 32, strand start mod 5)."""
    assert rstep % MASK_WORD == 1 and qstep % SEED_STEP == 1
    n, T = len(run_lens), 4 * max(run_lens) + 3
    assert qstep - T > 2 * MAX_GAP and rstep - T > 2 * MAX_GAP
    r0, q0 = 11, 3
    P = _Pair(seed, [r0 + n * rstep + 37], [q0 + n * qstep + qtail])
    for i, L in enumerate(run_lens):
        P.plant(0, r0 + i * rstep, 0, q0 + i * qstep, *_core(P.rng, L), strand=strand)
    ref, qry, pl = P.finish()
    assert len(pl) == 4 * n and all(m.len == run_lens[k // 4] for k, m in enumerate(pl))
    clusters = [_cluster(pl[4 * i:4 * i + 4]) for i in range(n)] if record else []
    return Case(name, 1, ref, qry, _same_everywhere(clusters), pl)


def phase_classes(case):
    """{(reference stream start mod 32, query strand stream start mod 5)} of the case's planted matches."""
    return {(m.r % MASK_WORD, m.q % SEED_STEP) for m in case.planted}


def _family1():
    out = [_sheet("sheet20_fwd", 101, 0, [20] * 160, 321, 301, 40, True)]
    for t in range(5):      # query lengths 0 .. 4 mod 5: the reverse strand's k-mer is read from the forward window len - 16 - q
        out.append(_sheet(f"sheet20_rev_len{t}", 110 + t, 1, [20] * 160, 321, 301, 40 + t, True))
    assert {len(c.qry[0][1]) % 5 for c in out[1:]} == set(range(5))
    for c in out:
        assert len(phase_classes(c)) == MASK_WORD * SEED_STEP, c.name
        assert {(m.r % MASK_WORD, m.q % SEED_STEP) for m in c.planted[::4]} == phase_classes(c), c.name      # the core starts alone cover it
    # 4 x 19 = 76 >= 65 matched bases, but no match reaches 20: nothing may be seeded
    out += [_sheet("sheet19_fwd", 121, 0, [19] * 160, 321, 301, 41, False), _sheet("sheet19_rev", 122, 1, [19] * 160, 321, 301, 43, False)]
    # runs of 21 .. 40: two to five sampled positions inside one match, every (length, strand start mod 5)
    long_runs = [21 + (i // 5) % 20 for i in range(100)]
    for name, seed, strand in (("sheet21to40_fwd", 131, 0), ("sheet21to40_rev", 132, 1)):
        c = _sheet(name, seed, strand, long_runs, 417, 401, 42 + strand, True)
        assert {(m.len, m.q % SEED_STEP) for m in c.planted} == {(L, p) for L in range(21, 41) for p in range(5)}, name
        out.append(c)
    return out


# ---- family 2: position edges ---------------------------------------------------------------------------------------
def _edge_pair(name, seed, strand, rspec, qspec):
    """One core; spec = ("start", k): begins at position k, ("end", d): ends d bases before the last one, ("mid",)."""
    P = _Pair(seed, [331], [347])
    rt, qt = _core(P.rng, 20)
    T = len(rt)

    def pos(spec, n):
        return spec[1] if spec[0] == "start" else n - T - spec[1] if spec[0] == "end" else 120
    P.plant(0, pos(rspec, 331), 0, pos(qspec, 347), rt, qt, strand=strand)
    ref, qry, pl = P.finish()
    m0, m3 = pl[0], pl[3]
    if rspec[0] == "start":
        assert m0.r == rspec[1]
    if qspec[0] == "start":
        assert m0.q == qspec[1]
    if rspec[0] == "end":
        assert m3.r + m3.len == 331 - rspec[1]
    if qspec[0] == "end":
        assert m3.q + m3.len == 347 - qspec[1]
    return Case(name, 2, ref, qry, _same_everywhere([_cluster(pl)]), pl)


N_VARIANTS = [(n, side, where) for n in (1, 5) for side in ("after", "before") for where in ("ref", "qry")]


def _n_pair(name, seed, strand):
    """Cores directly after / before a single N and a run of five, in the reference or in the query strand."""
    T = 83
    P = _Pair(seed, [200 + len(N_VARIANTS) * 321 + 60], [180 + len(N_VARIANTS) * 301 + 51])
    for j, (n, side, where) in enumerate(N_VARIANTS):
        rp, sp = 200 + j * 321, 180 + j * 301
        at = -n if side == "after" else T
        if where == "ref":
            P.put_ref(0, rp + at, "N" * n)
        else:
            P.put_strand(0, sp + at, "N" * n, strand)
        P.plant(0, rp, 0, sp, *_core(P.rng, 20), strand=strand)
    ref, qry, pl = P.finish()
    R, S = ref[0][1], qry[0][1] if strand == 0 else revcomp(qry[0][1])
    for j, (n, side, where) in enumerate(N_VARIANTS):
        first, last = pl[4 * j], pl[4 * j + 3]
        text, p = (R, first.r if side == "after" else last.r + last.len) if where == "ref" else (S, first.q if side == "after" else last.q + last.len)
        assert (text[p - n:p] if side == "after" else text[p:p + n]) == "N" * n, (name, j)
    return Case(name, 2, ref, qry, _same_everywhere([_cluster(pl[4 * j:4 * j + 4]) for j in range(len(N_VARIANTS))]), pl)


def _record_edge_pair(name, seed, strand):
    """Cores on the first and on the last base of a record, on either side, beside records shorter than a match and empty records."""
    T = 83
    rl, ql = [15, 620, 0, 640, 10], [600, 12, 0, 610, 17]
    P = _Pair(seed, rl, ql)
    spots = [(1, 0, 0, 250), (1, rl[1] - T, 3, 260), (1, 270, 0, 0), (3, 0, 3, 0), (3, rl[3] - T, 3, ql[3] - T), (3, 280, 0, ql[0] - T)]
    for rrec, rp, qrec, sp in spots:
        P.plant(rrec, rp, qrec, sp, *_core(P.rng, 20), strand=strand)
    ref, qry, pl = P.finish()
    assert any(m.rpos == 0 for m in pl) and any(m.rpos + m.len == rl[m.rrec] for m in pl)
    assert any(m.qpos == 0 for m in pl) and any(m.qpos + m.len == ql[m.qrec] for m in pl)
    return Case(name, 2, ref, qry, _same_everywhere([_cluster(pl[4 * j:4 * j + 4]) for j in range(len(spots))]), pl)


def _family2():
    out, seed = [], 2000
    for strand in (0, 1):
        s = "fwd" if strand == 0 else "rev"
        for kind in ("start", "end"):
            for k in range(6):
                for where, rspec, qspec in (("ref", (kind, k), ("mid",)), ("qry", ("mid",), (kind, k)), ("both", (kind, k), (kind, k))):
                    seed += 1
                    out.append(_edge_pair(f"{kind}{k}_{where}_{s}", seed, strand, rspec, qspec))
        out.append(_n_pair(f"beside_n_{s}", 2900 + strand, strand))
        out.append(_record_edge_pair(f"record_edges_{s}", 2950 + strand, strand))
    return out


FAMILY2_MIN = 2 * (2 * 6 * 3 + 2)


# ---- families 3, 4: join thresholds, minimum cluster ----------------------------------------------------------------
def _chain_pair(name, family, seed, strand, lens, qgaps, rgaps, joined_ab, joined_ba):
    """Exact matches of the given lengths in one record each side, with the given gaps between them in the query strand and in the reference."""
    P = _Pair(seed, [130 + sum(lens) + sum(rgaps) + 170], [100 + sum(lens) + sum(qgaps) + 163])
    rp, sp = 130, 100
    for k, L in enumerate(lens):
        P.plant(0, rp, 0, sp, "".join(P.rng.choice("ACGT") for _ in range(L)), strand=strand)
        if k + 1 < len(lens):
            rp, sp = rp + L + rgaps[k], sp + L + qgaps[k]
    ref, qry, pl = P.finish()
    assert [m.len for m in pl] == list(lens)
    for k in range(len(lens) - 1):
        a, b = pl[k], pl[k + 1]
        assert b.q - (a.q + a.len) == qgaps[k] and b.r - (a.r + a.len) == rgaps[k]
        assert abs((b.q - b.r) - (a.q - a.r)) == abs(qgaps[k] - rgaps[k])
    exp = {(mm, sw): ([_cluster(pl)] if j else []) for mm in (False, True) for sw, j in ((False, joined_ab), (True, joined_ba))}
    return Case(name, family, ref, qry, exp, pl)


def _split_query_records_pair(name, seed, strand):
    """Two 40-base matches 30 bases apart on one diagonal of the streams — but in two query records: they must not join.  With B as
    the reference they do (the reference is one text to mgaps), and postnuc cuts the cluster at the record junction: two records."""
    P = _Pair(seed, [400], [214, 215])
    first, second = (0, 1) if strand == 0 else (1, 0)      # the strand stream lists the records of the reverse strand last to first
    P.plant(0, 100, first, len(P.seq[1][first]) - 40 - 14, "".join(P.rng.choice("ACGT") for _ in range(40)), strand=strand)
    P.plant(0, 170, second, 15, "".join(P.rng.choice("ACGT") for _ in range(40)), strand=strand)
    ref, qry, pl = P.finish()
    a, b = pl
    assert b.q - (a.q + a.len) == 30 == b.r - (a.r + a.len) and a.qrec != b.qrec
    exp = {(mm, False): [] for mm in (False, True)}
    exp.update({(mm, True): [_cluster([a]), _cluster([b])] for mm in (False, True)})
    return Case(name, 3, ref, qry, exp, pl)


def _family3():
    out, seed = [], 3000
    for strand in (0, 1):
        s = "fwd" if strand == 0 else "rev"
        for sep, dd, j in JOIN_TABLE:
            for side, sign in (("ref_longer", 1), ("qry_longer", -1)):
                if dd == 0 and sign < 0:
                    continue
                seed += 1
                rgap = sep + sign * dd      # with B as the reference the separation is measured on A
                out.append(_chain_pair(f"sep{sep}_dd{dd}_{side}_{s}", 3, seed, strand, (40, 40), (sep,), (rgap,), bool(j), joins(rgap, dd)))
        out.append(_split_query_records_pair(f"two_query_records_{s}", 3900 + strand, strand))
    return out


FAMILY3_MIN = 2 * (sum(1 if dd == 0 else 2 for _, dd, _ in JOIN_TABLE) + 1)


def _family4():
    out, seed = [], 4000
    for strand in (0, 1):
        for lens, j in MIN_CLUSTER_TABLE:
            seed += 1
            gaps = (30,) * (len(lens) - 1)
            out.append(_chain_pair("len_" + "_".join(map(str, lens)) + ("_fwd" if strand == 0 else "_rev"), 4, seed, strand, lens, gaps, gaps, bool(j), bool(j)))
    return out


FAMILY4_MIN = 2 * len(MIN_CLUSTER_TABLE)


# ---- family 5: MUM uniqueness ---------------------------------------------------------------------------------------
MUM_KINDS = ["ref_twice_one_record", "ref_twice_two_records", "qry_twice_one_record", "qry_once_in_two_records", "one_run_twice_in_ref"]


def _mum_case(kind, seed, strand):
    name = kind + ("_fwd" if strand == 0 else "_rev")
    two_r, two_q = kind == "ref_twice_two_records", kind == "qry_once_in_two_records"
    P = _Pair(seed, [400, 410] if two_r else [720], [390, 420] if two_q else [730])
    rt, qt = _core(P.rng, 20)
    if kind.startswith("ref_twice"):
        spots = [(0, 120, 0, 150), (1, 160, 0, 150) if two_r else (0, 430, 0, 150)]
    elif kind.startswith("qry"):
        spots = [(0, 120, 0, 150), (0, 120, 1, 190) if two_q else (0, 120, 0, 460)]
    else:
        spots = [(0, 120, 0, 150)]
    for rrec, rp, qrec, sp in spots:
        P.plant(rrec, rp, qrec, sp, rt, qt, strand=strand)
    if kind == "one_run_twice_in_ref":
        P.plant(0, 450, 0, 150 + 21, rt[21:41], strand=strand)      # the core's second run once more, far off its diagonal
    ref, qry, pl = P.finish()
    copies = [_cluster(pl[4 * k:4 * k + 4]) for k in range(len(spots))]
    # --mum: a match must be unique in the whole reference and in its own query record
    mum = {"ref_twice_one_record": ([], []), "ref_twice_two_records": ([], copies), "qry_twice_one_record": ([], []),
           "qry_once_in_two_records": (copies, []), "one_run_twice_in_ref": ([], [])}[kind]      # three unique runs: 60 < 65
    exp = {(False, False): mum[0], (False, True): mum[1], (True, False): copies, (True, True): copies}
    return Case(name, 5, ref, qry, exp, pl)


def _family5():
    return [_mum_case(kind, 5000 + 10 * strand + k, strand) for strand in (0, 1) for k, kind in enumerate(MUM_KINDS)]


# ---- family 6: many clusters in one unit ----------------------------------------------------------------------------
def _many(name, seed, strand):
    """MANY_CLUSTERS pairs of 40-base matches in one (pair, strand) unit, cycling through MANY_FORMS; the longer gap is the reference's."""
    rstep, qstep = 331, 311
    P = _Pair(seed, [150 + MANY_CLUSTERS * rstep], [120 + MANY_CLUSTERS * qstep])
    for i in range(MANY_CLUSTERS):
        sep, dd = MANY_FORMS[i % 4]
        for rp, sp in ((150 + i * rstep, 120 + i * qstep), (150 + i * rstep + 40 + sep + dd, 120 + i * qstep + 40 + sep)):
            P.plant(0, rp, 0, sp, "".join(P.rng.choice("ACGT") for _ in range(40)), strand=strand)
    ref, qry, pl = P.finish()
    assert len(pl) == 2 * MANY_CLUSTERS >= 600 and max(len(ref[0][1]), len(qry[0][1])) < 150_000
    exp = {(mm, sw): [] for mm in (False, True) for sw in (False, True)}
    for i in range(MANY_CLUSTERS):
        a, b = pl[2 * i], pl[2 * i + 1]
        sep, dd = MANY_FORMS[i % 4]
        assert b.q - (a.q + a.len) == sep and abs((b.q - b.r) - (a.q - a.r)) == dd and b.r - (a.r + a.len) == sep + dd
        if i:
            assert a.q - (pl[2 * i - 1].q + 40) > MAX_GAP and a.r - (pl[2 * i - 1].r + 40) > MAX_GAP
        for mm in (False, True):
            if joins(sep, dd):
                exp[(mm, False)].append(_cluster([a, b]))
            if joins(sep + dd, dd):
                exp[(mm, True)].append(_cluster([a, b]))
    assert len(exp[(False, False)]) == MANY_CLUSTERS // 2
    return Case(name, 6, ref, qry, exp, pl)


def _family6():
    return [_many("many_fwd", 6001, 0), _many("many_rev", 6002, 1)]


FAMILY_MIN = {1: 1 + 5 + 2 + 2, 2: FAMILY2_MIN, 3: FAMILY3_MIN, 4: FAMILY4_MIN, 5: 2 * len(MUM_KINDS), 6: 2}
# what the sheets of family 1 and the joining clusters of family 6 alone claim, over two modes and two directions
RECORD_FLOOR = 4 * (6 * 160 + 2 * 100) + 4 * 2 * (MANY_CLUSTERS // 2)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = _family1() + _family2() + _family3() + _family4() + _family5() + _family6()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert set(c.expect) == {(mm, sw) for mm in (False, True) for sw in (False, True)}, c.name
        assert max(sum(len(s) for _, s in g) for g in (c.ref, c.qry)) < 150_000, c.name
    return tuple(cases)


def claimed_records(cases):
    """The floor of the suite: how many records the claims of all cases, modes and directions hold."""
    return sum(len(v) for c in cases for v in c.expect.values())


# ---- files, the oracle, and holding records against a claim ----------------------------------------------------------
def write_case(dirpath, case):
    """(path of A, path of B): the FASTA files the oracle, the statement and Engine.add_fasta read."""
    paths = []
    for tag, recs in (("a", case.ref), ("b", case.qry)):
        p = dirpath / f"{case.name}_{tag}.fna"
        with open(p, "w") as fh:
            for rid, s in recs:
                fh.write(f">{rid}\n")
                fh.write("".join(s[i:i + 70] + "\n" for i in range(0, len(s), 70)) or "\n")
        paths.append(p)
    return tuple(paths)


def parse_records(stdout, with_indels=False):
    """{(ref id, qry id, rs, re, qs, qe, errors): indel list} of the oracle's / the statement's ALN lines."""
    recs, cur = {}, None
    for line in stdout.splitlines():
        t = line.split()
        if t and t[0] == "ALN":
            cur = (t[1], t[2], int(t[3]), int(t[4]), int(t[5]), int(t[6]), int(t[7]))
            recs[cur] = []
        elif with_indels and cur is not None and len(t) == 1 and t[0] != "0":
            recs[cur].append(int(t[0]))
    return recs


def run_all(jobs, workers=8):
    """jobs: {key: argv}; runs them (a few at a time) and returns {key: CompletedProcess}."""
    keys = list(jobs)
    with ThreadPoolExecutor(max_workers=workers) as pool:
        done = list(pool.map(lambda k: subprocess.run([str(x) for x in jobs[k]], capture_output=True, text=True), keys))
    return dict(zip(keys, done))


def oracle_records(oracle_exe, paths):
    """{(case name, maxmatch, swapped): {record: indel list}} for paths = {case name: (path of A, path of B)}."""
    jobs = {}
    for name, (pa, pb) in paths.items():
        for mm in (False, True):
            for sw in (False, True):
                jobs[(name, mm, sw)] = [oracle_exe] + ([pb, pa] if sw else [pa, pb]) + ["--delta"] + (["--maxmatch"] if mm else [])
    out = {}
    for key, r in run_all(jobs).items():
        assert r.returncode == 0, (key, r.stderr[-300:])
        out[key] = parse_records(r.stdout, True)
    return out


def claim_problems(case, maxmatch, swapped, records):
    """[] if the records are exactly the claim's clusters, one record each; otherwise what is missing and what is surplus."""
    ids = ([i for i, _ in case.ref], [i for i, _ in case.qry])
    left = set(records)
    problems = []
    for a_rec, a_lo, a_hi, b_rec, b_lo, b_hi, strand in case.expect[(maxmatch, swapped)]:
        if swapped:
            want = (ids[1][b_rec], ids[0][a_rec], b_lo, b_hi, a_lo, a_hi)
        else:
            want = (ids[0][a_rec], ids[1][b_rec], a_lo, a_hi, b_lo, b_hi)

        def holds(rec):
            lo, hi = min(rec[4], rec[5]), max(rec[4], rec[5])
            return (rec[0], rec[1]) == want[:2] and (rec[4] > rec[5]) == bool(strand) and rec[2] < rec[3] and \
                want[2] + 1 - SLACK <= rec[2] <= want[2] + 1 and want[3] <= rec[3] <= want[3] + SLACK and \
                want[4] + 1 - SLACK <= lo <= want[4] + 1 and want[5] <= hi <= want[5] + SLACK
        hits = [rec for rec in left if holds(rec)]
        if len(hits) == 1:
            left.discard(hits[0])
        else:
            problems.append(("no record for" if not hits else "several records for", want, "strand", strand))
    problems += [("surplus record", rec) for rec in sorted(left)]
    return problems
