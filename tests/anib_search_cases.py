"""Inputs and references shared by the ANIb search-mode tests (test_anib_search_cpu.py, test_anib_search_gpu.py) and by
tools/anib_search_probe.py: the six synthetic genomes, the host statement of fragment mode in either search mode, the independent
blastn oracle, and the constructed edge inputs.

The host statement (oracle/anib_cpu.cpp) switches on getenv("ANIB_ALL_DIAGS") at call time.  host_rows is the ONLY place that sets
the variable: it sets or removes it immediately before the call and removes it immediately after, so it is never set while a
default-mode comparison runs.  Every reference is computed once per process and handed out as is (callers do not modify the rows)."""
import os
import sys

import numpy as np

from tests.conftest import ROOT

for _p in (ROOT / "oracle", ROOT / "tools"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import anib_cpu  # noqa: E402
import blastn_oracle  # noqa: E402
import blastn_oracle_agreement as agreement  # noqa: E402
from anib_product_vs_oracle import side_by_side, tuples  # noqa: E402

SEED, N, L = 20250302, 6, 150_000
ENV = "ANIB_ALL_DIAGS"
FIELDS = ("frag", "length", "mismatch", "gaps", "nident", "qlen", "qstart", "qend", "sstart", "send", "srec", "score")
MODES = ("seeds", "all_diagonals")
DIVERGED = [(5, 4), (4, 5), (3, 5), (0, 5), (3, 4)]      # the pairs the mode changes rows of
ORACLE_PAIRS = [(5, 4), (4, 5), (3, 5)]
CLOSE = [(0, 1), (2, 3)]                                   # the pairs it leaves alone

_genomes = []
_host = {}
_oracle = {}


def genomes():
    """synth.genome(20250302, 6, g, 150_000) for g = 0 .. 5."""
    if not _genomes:
        from pyani_amd import synth
        _genomes.extend(synth.genome(SEED, N, g, L) for g in range(N))
    return _genomes


def rows_of(a):
    return [tuple(int(r[k]) for k in FIELDS) for r in a]


def host_pair(monkeypatch, query, subject, mode, fragsize=1020):
    """The host statement's table of one ordered pair in `mode`; the variable is gone again when this returns."""
    assert mode in MODES
    if mode == "all_diagonals":
        monkeypatch.setenv(ENV, "1")
    else:
        monkeypatch.delenv(ENV, raising=False)
    try:
        return anib_cpu.anib_cpu_pair(query, subject, fragsize)
    finally:
        monkeypatch.delenv(ENV, raising=False)
        assert ENV not in os.environ


def host_rows(monkeypatch, q, s, mode):
    """host_pair over genomes q, s of the six, cached."""
    key = (q, s, mode)
    if key not in _host:
        g = genomes()
        _host[key] = host_pair(monkeypatch, g[q], g[s], mode)
    return _host[key]


def oracle_used(q, s):
    """The rows parse_blast_tab uses of the independent blastn oracle's table, cached."""
    if (q, s) not in _oracle:
        g = genomes()
        _oracle[(q, s)] = agreement.used_rows(tuples(blastn_oracle.blastn_pair(g[q], g[s])))
    return _oracle[(q, s)]


def oracle_agreement(rows, q, s):
    """(used rows of the oracle, used rows of `rows` identical to them)."""
    rep = side_by_side(agreement.used_rows(tuples(rows)), oracle_used(q, s))
    return rep["used_rows_other"], rep["identical"]


# ---- constructed inputs ----------------------------------------------------------------------------------------------------
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def revcomp(seq):
    return _COMP[np.asarray(seq, dtype=np.uint8)[::-1]]


def mutate(seq, rng, sub_rate, indel_every=0):
    """A copy of `seq` (ACGT bytes) with a substitution at every position with probability sub_rate and, when indel_every > 0, a
    1-3-base insertion or deletion about once per indel_every bases."""
    seq = np.asarray(seq, dtype=np.uint8)
    out = []
    i = 0
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    while i < len(seq):
        if indel_every and rng.random() < 1.0 / indel_every:
            k = int(rng.integers(1, 4))
            if rng.random() < 0.5:
                out.extend(alphabet[rng.integers(0, 4, k)])      # insertion
            else:
                i += k                                            # deletion
                continue
        b = seq[i]
        if rng.random() < sub_rate:
            b = alphabet[(int(np.where(alphabet == b)[0][0]) + int(rng.integers(1, 4))) & 3]
        out.append(b)
        i += 1
    return np.array(out, dtype=np.uint8)


def one_record(seq):
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    return seq, np.array([0, len(seq)], dtype=np.uint64)


def ends_case():
    """(query, subject): the subject is a two-record genome of 2 x 20 kb; the query holds diverged copies (about 78 % identity by
    substitutions, about one 1-3-base indel per 150 bases) of its first 3 kb, its last 3 kb and the 3 kb straddling the record
    boundary, each in both orientations, one record per copy."""
    from pyani_amd import synth
    seq = np.ascontiguousarray(synth.genome(SEED, N, 0, 41_000)[0][:40_000], dtype=np.uint8)
    assert len(seq) == 40_000 and set(seq.tolist()) <= set(b"ACGT")
    subject = (seq, np.array([0, 20_000, 40_000], dtype=np.uint64))
    rng = np.random.default_rng(7)
    pieces = []
    for lo in (0, 37_000, 18_500):
        copy = mutate(seq[lo:lo + 3000], rng, 0.22, 150)
        pieces += [copy, revcomp(copy)]
    off = np.cumsum([0] + [len(p) for p in pieces]).astype(np.uint64)
    return (np.concatenate(pieces), off), subject


# The tandem duplication's unit length = the distance between the two candidates' diagonals.  At 70, 82 and 86 the host statement's
# final alignment bridges the duplication with one gap (one row with 72 / 84 / 86 gap bases: a gap of k costs 5 + 2 k, the X-drop is
# 166); from 90 on it cannot and fragment 2 has two rows.  Below 95 the second candidate's +-47 band still reaches into the first
# one's neighbourhood (+-47), which the "taken" rule cuts.
TANDEM_UNIT = 90


def tandem_case():
    """(query, subject): the subject is a 6 kb region with a TANDEM_UNIT-base tandem duplication in its middle, the query the
    region without the duplication, diverged to about 80 %: the alignment left of the duplication and the one right of it lie
    TANDEM_UNIT diagonals apart, so the second candidate's +-47 band overlaps the first one's neighbourhood."""
    from pyani_amd import synth
    anc = np.ascontiguousarray(synth.genome(SEED, N, 1, 7_000)[0][:6_000], dtype=np.uint8)
    assert len(anc) == 6_000 and set(anc.tolist()) <= set(b"ACGT")
    mid = 2_550      # the middle of fragment 2 (bases 2040 .. 3059)
    subject = np.concatenate([anc[:mid], anc[mid - TANDEM_UNIT:mid], anc[mid:]])
    query = mutate(anc, np.random.default_rng(11), 0.20, 0)
    return one_record(query), one_record(subject)
