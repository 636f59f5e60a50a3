"""Directed rectangles for the forced re-alignment ladder of the ANIm extender (pga_postnuc.inc: the narrow / wide / group / strips
kernels behind pg_anim_forced_rects), with what is expected of each: the error count of the plain-integer referee
(tools/anim_debug/forced_referee.h), the verdict and the certified-band ladder of the host statement (pgn::ScalarEngine's band loop,
logged by tools/anim_debug/forced_rects.cpp), and from the ladder the kernel class that takes every pass.

The span arithmetic and the window thresholds are RESTATED here, not imported: a pass at band w spans |M - N| + 2 w + 1 + 5
diagonals (N + M + 1 + 5 for the whole rectangle); a window of 64 DPL diagonals is sure to hold 62 DPL + 2 of them; the group of four
waves holds 256 DPL - 8.

What a rectangle can be.  The engines' score words have a floor at -2700 (pg_nucmer_core.h): a path whose prefix falls below it is
lost, and a rectangle whose corner stays unreachable is reported (status 2), not counted.  A deleted block of df bases costs 7 df - 3, so
"identical apart from one deleted block, certified by the first band" exists only while 3 (matching bases before the block's end) - 7 df
stays above the floor, and with sides of at most 10 000 bases that ends at df = 3269 (span 3331).  The boundary cases up to threshold
3064 are built that way (the block placed no earlier than the prefix allows); for the thresholds 4088, 6136 and 8184 the same
construction with a short side of 100 bases puts the FIRST pass on exactly that span and engine, the corner comes back unreachable,
the ladder doubles on to the whole rectangle and the expected verdict is status 2 — the referee's optimal path confirms that its prefix
lies below the floor.  Likewise a run has more than two passes only through the floor rule: a band that reaches the corner names a
band that is certain to certify (forced_band_after).  The hand-over cases say which rule moves them.
"""
import functools
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

FIRST_BAND = 28
FLOOR = -2700
THR_NARROW = (126, 250, 374, 498)              # windows of 128 / 256 / 384 / 512 diagonals (DPL 2, 4, 6, 8)
THR_WIDE = (498, 746, 994, 1490, 1986)         # 512 / 768 / 1024 / 1536 / 2048 (DPL 8, 12, 16, 24, 32)
THR_GROUP = (3064, 4088, 6136, 8184)           # four waves: 3072 / 4096 / 6144 / 8192 (DPL 12, 16, 24, 32 per wave)
DPL_NARROW, DPL_WIDE, DPL_GROUP = (2, 4, 6, 8), (8, 12, 16, 24, 32), (12, 16, 24, 32)
ALL_THRESHOLDS = tuple(sorted(set(THR_NARROW + THR_WIDE + THR_GROUP)))
KERNELS = ("narrow", "wide", "group", "strips")


def span_of(N, M, w):
    """Diagonals a pass needs in its window: the band (w < 0: the whole rectangle) and the window's margins."""
    return (N + M + 1 if w < 0 else abs(M - N) + 2 * w + 1) + 5


def dispatch(spans, win_max=2048, group_max=8184):
    """The (kernel, DPL) that takes each pass of ONE run, in order; a run never returns to an earlier kernel.  win_max / group_max: the
    development knobs PYANI_PN_WINDOW_MAX / PYANI_PN_GROUP_MAX.  DPL 0: the strips' column engine."""
    out, k = [], 0
    for s in spans:
        while True:
            if k == 0:
                fit = [d for d, t in zip(DPL_NARROW, THR_NARROW) if 64 * d <= win_max and s <= t]
                if win_max >= 128 and s <= THR_NARROW[-1] and fit:
                    out.append(("narrow", fit[0]))
                    break
            elif k == 1:
                fit = [d for d, t in zip(DPL_WIDE, THR_WIDE) if 64 * d <= win_max and s <= t]
                if fit:
                    out.append(("wide", fit[0]))
                    break
            elif k == 2:
                fit = [d for d, t in zip(DPL_GROUP, THR_GROUP) if s <= t]
                if s <= group_max and fit:
                    out.append(("group", fit[0]))
                    break
            else:
                out.append(("strips", 0))
                break
            k += 1
    return out


def counters_of(runs, win_max=2048, group_max=8184):
    """What pg_anim_counters shows after the runs (each a list of spans): passes[4] = out[27..30], the passes by span class as
    pn_forced_wave counts them (<= 256, <= 512, <= 2048, beyond; every pass of the group counts as beyond), and calls[4] = out[32 + 4 k],
    k = 4 .. 7: diagonal-engine calls in the narrow kernel, in the wide kernel's windows up to 1024 / up to 2048, in the group.  The strips
    make no diagonal-engine call: their passes are sum(passes) - sum(calls)."""
    passes, calls = [0, 0, 0, 0], [0, 0, 0, 0]
    for spans in runs:
        for s, (kern, dpl) in zip(spans, dispatch(spans, win_max, group_max)):
            cls = 0 if s <= 256 else 1 if s <= 512 else 2 if s <= 2048 else 3
            passes[3 if kern == "group" else cls] += 1
            if kern == "narrow":
                calls[0] += 1
            elif kern == "wide":
                calls[1 if dpl <= 16 else 2] += 1
            elif kern == "group":
                calls[3] += 1
    return passes, calls


# ---- sequences ------------------------------------------------------------------------------------------------------------------
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def substitute(rng, s, positions):
    t = list(s)
    for p in positions:
        t[p] = "ACGT"[("ACGT".index(t[p]) + 1 + int(rng.integers(0, 3))) & 3]
    return "".join(t)


def scatter(rng, s, n_sub, n_indel=0, indel_max=3):
    """n_sub substitutions and n_indel short insertions / deletions at random places."""
    s = substitute(rng, s, rng.choice(len(s), size=n_sub, replace=False))
    for _ in range(n_indel):
        p, k = int(rng.integers(1, len(s) - indel_max - 1)), int(rng.integers(1, indel_max + 1))
        s = s[:p] + (rand_seq(rng, k) + s[p:] if rng.integers(0, 2) else s[p + k:])
    return s


def runs_pair(rng, runs):
    """tools/anim_debug/forced_check.cpp's cases: +n = n matching bases, -n = n bases that differ."""
    a = rand_seq(rng, sum(abs(r) for r in runs))
    at, miss = 0, []
    for r in runs:
        if r < 0:
            miss += range(at, at - r)
        at += abs(r)
    return a, substitute(rng, a, miss)


class Case:
    """name, group, reference sequence, query sequence AS STORED (the forward strand), strand, rectangles (A0, A1, B0, B1: B in strand
    coordinates), and the claim: per rectangle the kernel of every pass, or None where the table claims only what `first` says —
    (span, kernel, DPL) of the first pass."""

    def __init__(self, name, group, a, b_strand, strand, rects, claim=None, first=None):
        self.name, self.group, self.a, self.strand = name, group, a, strand
        self.b = revcomp(b_strand) if strand else b_strand      # (b_strand: what the rectangles' B coordinates index)
        self.rects = [tuple(int(v) for v in r) for r in (rects if rects is not None else _whole(a, b_strand))]
        self.claim, self.first = claim, first


def _whole(a, b):
    return [(0, len(a) - 1, 0, len(b) - 1)]


def _boundary_cases():
    out, turn = [], 0
    for T in ALL_THRESHOLDS:
        for span in (T, T + 1):
            df = span - (2 * FIRST_BAND + 6)
            # (both orientations while the referee's whole rectangle is small; above that they alternate from span to span)
            for n_gt_m in ((True, False) if T < 1490 else (span % 2 == 0,)):
                rng = np.random.default_rng(1000 * span + n_gt_m)
                # the earliest the block may start: the matching prefix has to carry the gap's price above the floor (300 to spare)
                lo = max(0, -(-(7 * df - 2400) // 3))
                certifies = lo + 100 + df <= 10000
                mn = lo + 100 if certifies else 100
                pos = ("start", "middle", "end")[turn % 3]
                first = lo if certifies else 0
                off = {"start": first, "middle": (first + mn) // 2, "end": mn}[pos]
                common = rand_seq(rng, mn)
                long_ = common[:off] + rand_seq(rng, df) + common[off:]
                a, b = (long_, common) if n_gt_m else (common, long_)
                strand = 1 if turn % 4 == 3 else 0
                kern, dpl = dispatch([span])[0]
                out.append(Case(f"bnd_{span}_{pos}_{'NgtM' if n_gt_m else 'MgtN'}", "boundary", a, b, strand, _whole(a, b),
                                claim=[(kern,)] if certifies else None, first=(span, kern, dpl)))
                turn += 1
    return out


def _shifted(rng, P, t, S):
    """A = P + U + S', B = P + S' + V (|U| = |V| = t unrelated bases): the optimal path deletes U and inserts V, t diagonals off the
    corner-to-corner span; inside a band narrower than t every path runs through S' misaligned and falls below the floor."""
    p, s = rand_seq(rng, P), rand_seq(rng, S)
    return p + rand_seq(rng, t) + s, p + s + rand_seq(rng, t)


def _handover_cases():
    out = []
    # pass 1 at band 28 reaches the corner without a certificate; the band it names is certain to certify
    rng = np.random.default_rng(4101)      # narrow -> wide: 3000 bases, 14 % substitutions and a few short indels
    a = rand_seq(rng, 3000)
    out.append(Case("hand_narrow_wide", "handover", a, scatter(rng, a, 420, 6), 0, None, claim=[("narrow", "wide")]))
    rng = np.random.default_rng(4102)      # wide -> group: a deleted block of 1200 after 5000 bases, 13 % substitutions
    a = rand_seq(rng, 6000)
    b = scatter(rng, a, 780, 4)
    out.append(Case("hand_wide_group", "handover", a[:5000] + rand_seq(rng, 1200) + a[5000:], b, 1, None, claim=[("wide", "group")]))
    # the floor rule: the corner is unreachable inside the band, the next band comes from the bound or doubles
    rng = np.random.default_rng(4103)      # narrow -> wide, certified there: the path lies 40 diagonals off
    a, b = _shifted(rng, 10, 40, 900)
    out.append(Case("hand_floor_narrow_wide", "handover", a, b, 0, None, claim=[("narrow", "wide")]))
    rng = np.random.default_rng(4104)      # the same with the path 500 diagonals off: certified on the 1536-diagonal window
    a, b = _shifted(rng, 1200, 500, 1500)
    out.append(Case("hand_floor_narrow_wide1536", "handover", a, b, 1, None, claim=[("narrow", "wide")]))
    # (group -> strips inside one run: the boundary cases at 4088 ... 8184, whose ladders double from the group on to the strips)
    return out      # (rectangles: the whole sequences)


_TINY = (1, 2, 27, 28, 29)


def _tiny_cases():
    out = []
    for strand in (0, 1):
        rng = np.random.default_rng(4200 + strand)
        a = rand_seq(rng, 96)
        b = scatter(rng, a, 12)
        rects = []
        for rep in range(4):      # every (N, M) at four places, the first at position 0 and the last ending on the last base
            for n in _TINY:
                for m in _TINY:
                    a0 = {0: 0, 3: len(a) - n}.get(rep, int(rng.integers(0, len(a) - n + 1)))
                    b0 = {0: 0, 3: len(b) - m}.get(rep, min(len(b) - m, max(0, a0 + int(rng.integers(-2, 3)))))
                    rects.append((a0, a0 + n - 1, b0, b0 + m - 1))
        # w = 28 is the whole rectangle while max(N, M) <= 28; a side of 29 has one banded pass first unless that certifies
        out.append(Case(f"tiny_s{strand}", "tiny", a, b, strand, rects, claim=None))
    return out


def _ends_cases():
    out = []
    for res in (0, 1, 15, 16, 17, 31):
        for strand in (0, 1):
            rng = np.random.default_rng(4300 + 2 * res + strand)
            a = rand_seq(rng, 320 + res)
            b = scatter(rng, a[:150] + a[157:], 25, 2) + rand_seq(rng, 32)
            b = b[:352 + res] if len(b) >= 352 + res else b + rand_seq(rng, 352 + res - len(b))      # both lengths = res (mod 32)
            la, lb = len(a), len(b)
            rects = [(0, 280, 0, 275), (30, la - 1, 28, lb - 1), (0, la - 1, 0, lb - 1)]
            out.append(Case(f"ends_r{res}_s{strand}", "ends", a, b, strand, rects, claim=[("narrow",)] * 3))
    return out


def _nonacgt_cases():
    out = []
    for k, strand in enumerate((0, 1)):
        rng = np.random.default_rng(4400 + k)
        a = rand_seq(rng, 400)
        b = scatter(rng, a, 10, 1)
        inside = a[:200] + "N" + a[201:260] + "R" + a[261:]
        out.append(Case(f"nonacgt_inside_s{strand}", "nonacgt", inside, b[:180] + "N" + b[181:], strand, [(20, 380, 18, 379)], claim=[("narrow",)]))
        edge_a = "N" + a[1:399] + "N"
        edge_b = "N" + b[1:-1] + "N"
        out.append(Case(f"nonacgt_edges_s{strand}", "nonacgt", edge_a, edge_b, strand, _whole(edge_a, edge_b) + [(0, 300, 3, 298), (100, 399, 99, len(b) - 1)],
                        claim=[("narrow",)] * 3))
        run_a = a[:150] + "N" * 40 + a[190:]
        run_b = b[:260] + "N" * 70 + b[330:]
        out.append(Case(f"nonacgt_runs_s{strand}", "nonacgt", run_a, run_b, strand, _whole(run_a, run_b) + [(140, 200, 138, 205)], claim=None))
    rng = np.random.default_rng(4410)      # the same on a wide window: a deleted block of 700 and a run of 40 unclean bases after it
    common = rand_seq(rng, 1200)
    a = common[:900] + rand_seq(rng, 700) + common[900:1000] + "N" * 40 + common[1040:]
    out.append(Case("nonacgt_wide", "nonacgt", a, common, 0, _whole(a, common), claim=[("wide",)]))
    return out


# (shape, seed) of rectangles whose error count DEPENDS on the tie order: found by search with the referee's other orders
# (tools/anim_debug/forced_referee.h: order 2, DELETE > INSERT > MATCH, counts differently on every one of them; the CPU test asserts it).
# Low-complexity sequences, unrelated: many paths share the optimal score.  Spans 182 / 212 / 352: the 256- and 384-diagonal windows.
_TIE_SHAPES = {"w256_n": (230, 110), "w256_m": (90, 240), "w384": (420, 130)}
_TIE_SEEDS = (("w256_n", 333), ("w256_n", 1156), ("w256_n", 1405), ("w256_m", 1054), ("w384", 46), ("w384", 359), ("w384", 551), ("w384", 606))
_TIE_PROBS = ((.45, .1, .35, .1), (.4, .4, .1, .1), (.3, .3, .3, .1))


def tie_pair(shape, seed):
    N, M = _TIE_SHAPES[shape]
    rng = np.random.default_rng([5000, seed, N, M])
    p = _TIE_PROBS[seed % 3]
    return tuple("".join("ACGT"[i] for i in rng.choice(4, size=n, p=p)) for n in (N, M))


def _ties_cases():
    out = []
    pairs = [("homopolymer", "A" * 64, "A" * 59), ("homopolymer_sub", "A" * 30 + "C" + "A" * 33, "A" * 61),
             ("dinucleotide", "AC" * 40, "AC" * 37), ("dinucleotide_odd", "AC" * 40, "AC" * 18 + "A" + "AC" * 20),
             ("trinucleotide_sub", "ACG" * 30, "ACG" * 14 + "ATG" + "ACG" * 13)]
    for k, (name, a, b) in enumerate(pairs):
        for strand in (0, 1):
            out.append(Case(f"ties_{name}_s{strand}", "ties", a, b, strand, _whole(a, b) + [(1, len(a) - 2, 0, len(b) - 1)], claim=[("narrow",)] * 2))
    for k, (shape, seed) in enumerate(_TIE_SEEDS):      # the order-sensitive ones, strands alternating
        a, b = tie_pair(shape, seed)
        out.append(Case(f"ties_sensitive_{shape}_{seed}_s{k % 2}", "ties", a, b, k % 2, _whole(a, b), claim=[("narrow",)]))
    return out


def _floor_cases():
    out = []
    rng = np.random.default_rng(4601)
    a, b = runs_pair(rng, [20, -700, 1200])          # A: the optimal path's prefix falls to about -1650 and recovers: exact
    out.append(Case("floor_A_deep_dip", "floor", a, b, 0, _whole(a, b), claim=None))
    rng = np.random.default_rng(4602)
    a, b = runs_pair(rng, [20, -1500, 2500])         # B: below the floor on every path: status 2, no error count
    out.append(Case("floor_B_below_floor", "floor", a, b, 0, _whole(a, b), claim=[("narrow", "wide", "group", "group", "group")]))
    rng = np.random.default_rng(4603)
    a, b = runs_pair(rng, [49, -1] * 30)             # C: an ordinary rectangle
    out.append(Case("floor_C_ordinary", "floor", a, b, 0, _whole(a, b), claim=[("narrow",)]))
    return out


def _limit_cases():
    rng = np.random.default_rng(4700)      # the longest side one engine call aligns (MAX_ALIGNMENT_LENGTH) against 50 bases: far below the floor
    a = rand_seq(rng, 10000)
    return [Case("limit_longest_side", "limits", a, a[:50], 0, None, claim=None, first=(10012, "strips", 0))]


@functools.lru_cache(maxsize=None)
def cases():
    out = _boundary_cases() + _handover_cases() + _tiny_cases() + _ends_cases() + _nonacgt_cases() + _ties_cases() + _floor_cases() + _limit_cases()
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


GROUPS = ("boundary", "handover", "tiny", "ends", "nonacgt", "ties", "floor")      # (and "limits": one rectangle at the size limit)


# ---- the host statement ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_tool():
    """tools/anim_debug/forced_rects, built beside its source (kept out of git) and built again only when a source is newer."""
    src = ROOT / "tools" / "anim_debug" / "forced_rects.cpp"
    exe = src.with_suffix("")
    deps = [src, src.parent / "forced_referee.h"] + sorted((ROOT / "pyani_amd" / "csrc").glob("pg_*.h"))
    if not exe.exists() or any(d.stat().st_mtime > exe.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'pyani_amd' / 'csrc'}", f"-I{src.parent}", str(src), "-o", str(exe)], check=True)
    return exe


@functools.lru_cache(maxsize=None)
def expected():
    """{case name: [per rectangle: dict(ref_errors, ref_min, status, errors, ladder, diag_status, diag_errors, diag_ladder, loops_ok,
    spans, w_used)]} — computed once per session (the referee fills whole rectangles of up to 9 300 x 6 300 cells)."""
    cs = cases()
    text = [str(len(cs))]
    for c in cs:
        text += [f"{c.name} {c.strand} {len(c.rects)}", c.a, c.b] + [" ".join(map(str, r)) for r in c.rects]
    out = subprocess.run([str(host_tool())], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout
    by_name = {c.name: c for c in cs}
    res = {c.name: [None] * len(c.rects) for c in cs}
    for ln in out.splitlines():
        f = ln.split()
        name, k = f[0], int(f[1])
        assert f[2] == "ref" and f[6] == "scalar"
        n1 = int(f[9])
        d = 10 + n1
        assert f[d] == "diag"
        n2 = int(f[d + 3])
        assert f[d + 4 + n2] == "loops" and f[d + 6 + n2] == "alt"
        A0, A1, B0, B1 = by_name[name].rects[k]
        N, M = A1 - A0 + 1, B1 - B0 + 1
        ladder = [int(v) for v in f[10:10 + n1]]
        status = int(f[7])
        res[name][k] = dict(N=N, M=M, ref_errors=int(f[4]), ref_min=int(f[5]), status=status, errors=int(f[8]), ladder=ladder,
                            diag_status=int(f[d + 1]), diag_errors=int(f[d + 2]), diag_ladder=[int(v) for v in f[d + 4:d + 4 + n2]],
                            loops_ok=f[d + 5 + n2] == "1", alt_errors=(int(f[d + 7 + n2]), int(f[d + 8 + n2])), spans=[span_of(N, M, w) for w in ladder],
                            w_used=0 if status == 2 else ladder[-1])
    assert all(r is not None for rs in res.values() for r in rs)
    return res


def list_call(strand, seed=77):
    """One pair of sequences holding every case of one strand back to back, and all their rectangles in shuffled order:
    (reference, query as stored, rectangles, [(case name, index)])."""
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
    rects, who = [], []
    for c in cs:
        for k, (A0, A1, B0, B1) in enumerate(c.rects):
            rects.append((A0 + a_off[c.name], A1 + a_off[c.name], B0 + b_off[c.name], B1 + b_off[c.name]))
            who.append((c.name, k))
    perm = np.random.default_rng(seed + strand).permutation(len(rects))
    return a, b, [rects[i] for i in perm], [who[i] for i in perm]
